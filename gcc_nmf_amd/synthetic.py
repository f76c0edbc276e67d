"""Seeded synthetic stereo mixtures of the benchmark shape.

Three low-passed, slowly amplitude-modulated noise sources; the right channel holds
integer-sample delayed copies (TDOA peak at tau = -delay/sampleRate); independent sensor
noise keeps |X| > 0 in every bin (no NaN coherence); samples are int16-representable
float32 so the data could have come from a wav file (wavfile.pcm2float convention).
Pure NumPy/SciPy input generation -- no part of the measured path.
"""
import numpy as np


def synthetic_mixture(fileIndex, numSamples=160000, sampleRate=16000, delays=(-20, 3, 27)):
    from scipy.signal import butter, lfilter
    rng = np.random.default_rng(20260925 + fileIndex)
    t = np.arange(numSamples) / float(sampleRate)
    b, a = butter(4, 4000.0 / (sampleRate / 2.0))
    left = np.zeros(numSamples)
    right = np.zeros(numSamples)
    for j, d in enumerate(delays):
        s = lfilter(b, a, rng.standard_normal(numSamples))
        phi = rng.uniform(0, 2 * np.pi)
        s = s * 0.5 * (1 + np.sin(2 * np.pi * (0.7 + 0.3 * j) * t + phi))
        left += s
        right += np.roll(s, d)
    left += rng.normal(0, 1e-3, numSamples)
    right += rng.normal(0, 1e-3, numSamples)
    x = np.stack([left, right])
    x = x / np.max(np.abs(x)) * 0.1
    pcm = np.round(x * 32768).astype(np.int16)
    return ((pcm.astype('float32') - 0) / 32768).astype(np.float32)


def synthetic_batch(firstIndex, count, numSamples=160000, sampleRate=16000):
    return np.stack([synthetic_mixture(firstIndex + i, numSamples, sampleRate) for i in range(count)])


def moving_source_mixture(seed, numSamples=96000, sampleRate=16000, staticDelay=-25, movingDelays=(5, 30), bandHz=250.0,
                          lowHz=250.0, highHz=6000.0, returnSources=False):
    """A talker who changes seat: two slowly amplitude-modulated noise sources in interleaved ``bandHz``-wide bands between ``lowHz``
    and ``highHz`` (counted from ``lowHz``, source 1 takes the even bands and source 0 the odd ones).  Source 0 stays put -- the right channel holds roll(s0,
    staticDelay) -- and source 1 jumps at the midpoint: roll(s1, movingDelays[0]) in the first half of the file, roll(s1,
    movingDelays[1]) in the second.  At 16 kHz, 1 m and 128 TDOAs the defaults put source 0 at index 97 and source 1 at 56 / 57, then
    23.  Sensor noise and int16-representable float32 samples as in synthetic_mixture.  ``returnSources``: also the two sources' left-
    channel images (2, numSamples), float64, on the mixture's scale -- what a separated left channel is scored against."""
    rng = np.random.default_rng(20261017 + seed)
    t = np.arange(numSamples) / float(sampleRate)
    freqs = np.fft.rfftfreq(numSamples, 1.0 / sampleRate)
    band = np.floor((freqs - lowHz) / bandHz).astype(int)
    inside = (freqs >= lowHz) & (freqs < highHz)
    half = numSamples // 2
    sources, right = [], np.zeros(numSamples)
    for j in range(2):
        spectrum = np.fft.rfft(rng.standard_normal(numSamples)) * (inside & (band % 2 == 1 - j))
        s = np.fft.irfft(spectrum, numSamples)
        phi = rng.uniform(0, 2 * np.pi)
        s = s * 0.5 * (1 + np.sin(2 * np.pi * (0.7 + 0.3 * j) * t + phi))
        sources.append(s)
        if j == 0:
            right += np.roll(s, staticDelay)
        else:
            right[:half] += np.roll(s, movingDelays[0])[:half]
            right[half:] += np.roll(s, movingDelays[1])[half:]
    sigma = 1e-2 * np.std(sources[0] + sources[1])
    x = np.stack([sources[0] + sources[1] + rng.normal(0, sigma, numSamples), right + rng.normal(0, sigma, numSamples)])
    scale = 0.1 / np.max(np.abs(x))
    pcm = np.round(x * scale * 32768).astype(np.int16)
    x = (pcm.astype('float32') / 32768).astype(np.float32)
    return (x, np.stack(sources) * scale) if returnSources else x


def reverberant_mixture(seed, numSamples=96000, sampleRate=16000, delays=(-20, 3, 27), responseMs=3.0, reverbGain=0.4,
                        returnSources=False):
    """Three talkers in a (slightly) reverberant room: low-passed noise sources with syllable-rate on/off envelopes, each convolved per
    channel with its own short seeded decaying impulse response (a unit direct path followed by ``responseMs`` of exponentially decaying
    noise, ``reverbGain`` at its start) on top of the integer delay of its right channel.  The two channels of a source are therefore
    not delayed copies of each other: its spatial covariance has full rank in every bin, which is what the spatial reconstruction
    models and a per-channel mask cannot use.  No sensor noise: the int16 rounding is the noise floor.  int16-representable float32
    samples as in synthetic_mixture.  ``returnSources``: also the sources' stereo images (3, 2, numSamples), float64, on the mixture's
    scale; they add up to the mixture before it is rounded to int16."""
    from scipy.signal import butter, lfilter
    rng = np.random.default_rng(20261018 + seed)
    t = np.arange(numSamples) / float(sampleRate)
    b, a = butter(4, 4000.0 / (sampleRate / 2.0))
    taps = max(2, int(round(responseMs * 1e-3 * sampleRate)))
    decay = np.exp(-np.arange(1, taps) / (taps / 4.0))
    images = []
    for j, d in enumerate(delays):
        s = lfilter(b, a, rng.standard_normal(numSamples))
        phi = rng.uniform(0, 2 * np.pi)
        s = s * (0.5 * (1 + np.sin(2 * np.pi * (2.0 + 0.7 * j) * t + phi))) ** 4
        h = [np.concatenate([[1.0], reverbGain * decay * rng.standard_normal(taps - 1)]) for _ in range(2)]
        images.append(np.stack([np.convolve(s, h[0])[:numSamples], np.roll(np.convolve(s, h[1])[:numSamples], d)]))
    images = np.stack(images)
    x = images.sum(axis=0)
    scale = 0.1 / np.max(np.abs(x))
    pcm = np.round(x * scale * 32768).astype(np.int16)
    x = (pcm.astype('float32') / 32768).astype(np.float32)
    return (x, images * scale) if returnSources else x


def speech_in_noise_mixture(seed, snrDb, numSamples=64000, sampleRate=16000, delay=12, bandCentresHz=(300.0, 700.0, 1200.0, 2000.0, 3000.0),
                            bandWidthHz=160.0, noiseCutoffHz=3000.0):
    """One talker against diffuse noise -- the offline speech-enhancement case.  The talker: one ``bandWidthHz``-wide band of noise at
    each of ``bandCentresHz``, each with its own squared half-sine syllabic envelope sin^2(pi r t + phi) (r = 2.5, 3.1, ... syllables
    per second); the right channel holds roll(talker, delay), so at 16 kHz, 1 m and 128 TDOAs the default puts the talker near index
    47.  The noise: independent ``noiseCutoffHz`` low-passed Gaussian noise in each channel (no direction), scaled so that the stereo
    talker-to-noise energy ratio is ``snrDb``.  int16-representable float32 samples as in synthetic_mixture.
    Returns (mixture (2, numSamples) float32, clean talker (2, numSamples) float64 on the mixture's scale)."""
    from scipy.signal import butter, lfilter
    rng = np.random.default_rng(20261019 + seed)
    t = np.arange(numSamples) / float(sampleRate)
    freqs = np.fft.rfftfreq(numSamples, 1.0 / sampleRate)
    talker = np.zeros(numSamples)
    for j, centre in enumerate(bandCentresHz):
        s = np.fft.irfft(np.fft.rfft(rng.standard_normal(numSamples)) * (np.abs(freqs - centre) < bandWidthHz / 2.0), numSamples)
        phi = rng.uniform(0, np.pi)
        talker += s / np.std(s) * np.sin(np.pi * (2.5 + 0.6 * j) * t + phi) ** 2
    clean = np.stack([talker, np.roll(talker, delay)])
    b, a = butter(4, noiseCutoffHz / (sampleRate / 2.0))
    noise = np.stack([lfilter(b, a, rng.standard_normal(numSamples)) for _ in range(2)])
    noise *= np.sqrt(np.sum(clean ** 2) / np.sum(noise ** 2) * 10.0 ** (-snrDb / 10.0))
    x = clean + noise
    scale = 0.1 / np.max(np.abs(x))
    pcm = np.round(x * scale * 32768).astype(np.int16)
    return (pcm.astype('float32') / 32768).astype(np.float32), clean * scale


def array_mixture(seed, microphonePositions, azimuthsDeg, numSamples=16000, sampleRate=16000, returnImages=False,
                  speedOfSound=340.29):
    """Far-field talkers in front of a microphone array: one low-passed noise source with a syllable-rate on/off envelope per azimuth
    (as ``reverberant_mixture`` builds its talkers), arriving from the unit vector u = (cos az, sin az, 0).  Microphone m at position
    r_m hears the talker delayed by -r_m . u / c -- applied as a circular phase ramp in the frequency domain, so fractional delays are
    exact -- plus a little independent sensor noise; int16-representable float32 samples as in synthetic_mixture.  Returns the mixture
    (M, numSamples) float32; with ``returnImages`` also the per-talker, per-channel images (J, M, numSamples), float64, on the
    mixture's scale (they add up to the mixture before the sensor noise and the int16 rounding)."""
    from scipy.signal import butter, lfilter
    r = np.asarray(microphonePositions, np.float64)
    if r.ndim != 2 or r.shape[1] != 3:
        raise ValueError('microphonePositions must have shape (M, 3), got %s' % (r.shape,))
    rng = np.random.default_rng(20261021 + seed)
    t = np.arange(numSamples) / float(sampleRate)
    freqs = np.fft.rfftfreq(numSamples, 1.0 / sampleRate)
    b, a = butter(4, 4000.0 / (sampleRate / 2.0))
    images = []
    for j, az in enumerate(np.deg2rad(np.asarray(azimuthsDeg, np.float64))):
        s = lfilter(b, a, rng.standard_normal(numSamples))
        phi = rng.uniform(0, 2 * np.pi)
        s = s * (0.5 * (1 + np.sin(2 * np.pi * (2.0 + 0.7 * j) * t + phi))) ** 4
        u = np.array([np.cos(az), np.sin(az), 0.0])
        delays = -r.dot(u) / float(speedOfSound)
        spectrum = np.fft.rfft(s)
        images.append(np.stack([np.fft.irfft(spectrum * np.exp(-2j * np.pi * freqs * d), numSamples) for d in delays]))
    images = np.stack(images)
    x = images.sum(axis=0)
    x = x + rng.normal(0, 1e-2 * np.std(x), x.shape)
    scale = 0.1 / np.max(np.abs(x))
    pcm = np.round(x * scale * 32768).astype(np.int16)
    x = (pcm.astype('float32') / 32768).astype(np.float32)
    return (x, images * scale) if returnImages else x
