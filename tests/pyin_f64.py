"""Float64 numpy restatement of pYIN pitch tracking as the reference calls it (test oracle only).

The reference takes pitch from `librosa.pyin` (librosa 0.10.0.post2, numpy 1.23.3, scipy 1.9.1; vits/data/audio.py:24-63).
librosa is not a dependency of this project, so this file restates its algorithm step by step; the numbers in the comments
are the steps of the arithmetic contract in DESIGN 3.1 (unpinned #5): parity with librosa itself is UNPINNED.  It shares no
code with vcvits_amd/ops/pitch.py beyond the scipy table calls.  Dense 1202 x 1202 Viterbi: ~0.35 s per second of audio.
"""
import numpy as np
import scipy.signal
import scipy.stats

SR = 16000
FRAME = 2048             # frame_length = win_length of the call sites
HOP = 320                # hard-coded at every call site
FMIN = 440.0 * 2.0 ** ((36 - 69) / 12.0)   # note_to_hz('C2')
FMAX = 440.0 * 2.0 ** ((96 - 69) / 12.0)   # note_to_hz('C7')
TINY = np.finfo(np.float64).tiny


def consts(sr=SR, frame_length=FRAME, hop_length=HOP, fmin=FMIN, fmax=FMAX):
    win = frame_length // 2
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - win - 1)
    n_bins_per_semitone = int(np.ceil(1.0 / 0.1))
    n_pitch_bins = int(np.floor(12 * n_bins_per_semitone * np.log2(fmax / fmin))) + 1
    max_semitones = round(35.92 * 12 * hop_length / sr)
    width = max_semitones * n_bins_per_semitone + 1
    return dict(win=win, min_period=min_period, max_period=max_period, n_pitch_bins=n_pitch_bins, width=width,
                bins_per_semitone=n_bins_per_semitone)


def reflect_index(p, n, pad):
    """Index into the unpadded signal of padded position p (numpy's 'reflect', repeated when pad >= n; n >= 2)."""
    q = np.abs(np.asarray(p, dtype=np.int64) - pad)
    period = 2 * (n - 1)
    r = q % period
    return np.where(r >= n, period - r, r)


def frames(y, pad, frame_length=FRAME, hop_length=HOP):
    """1. Reflect padding (a copy) and framing: [F, frame_length] float32."""
    y = np.asarray(y, dtype=np.float32)
    if not np.all(np.isfinite(y)):
        raise ValueError("audio buffer is not finite everywhere")
    n = y.shape[0]
    if n + 2 * pad < frame_length or n < 2:
        raise ValueError("input is too short for frame_length=%d" % frame_length)
    yp = y[reflect_index(np.arange(n + 2 * pad), n, pad)]
    nf = 1 + (yp.shape[0] - frame_length) // hop_length
    idx = np.arange(nf)[:, None] * hop_length + np.arange(frame_length)[None, :]
    return yp[idx]


def cmndf(fr, c):
    """2.-4. fp64 FFT autocorrelation, float32 energy, the difference function and its cumulative-mean normalisation.
    fr [F, frame_length] float32 -> [F, max_period - min_period + 1] float64."""
    L = fr.shape[1]
    win, lo, hi = c["win"], c["min_period"], c["max_period"]
    f64 = fr.astype(np.float64)                                    # 2. numpy 1.23's rfft upcasts float32 to float64
    a = np.fft.rfft(f64, L, axis=1)
    b = np.fft.rfft(f64[:, win:0:-1], L, axis=1)
    acf = np.fft.irfft(a * b, L, axis=1)[:, win:]
    acf[np.abs(acf) < 1e-6] = 0
    cs = np.cumsum(fr * fr, axis=1, dtype=np.float32)              # 3. float32 squares, sequential float32 prefix
    energy = cs[:, win:] - cs[:, :-win]
    energy[np.abs(energy) < np.float32(1e-6)] = 0
    d = (energy[:, :1] + energy).astype(np.float64) - 2 * acf      # 4. float32 first sum, then fp64
    num = d[:, lo:hi + 1]
    cum = np.cumsum(d[:, 1:hi + 1], axis=1) / np.arange(1, hi + 1)  # sequential fp64 cumulative sum
    den = cum[:, lo - 1:hi]
    return num / (den + TINY)


def parabolic_shifts(x):
    """5. Parabolic interpolation along the last axis; end elements 0."""
    out = np.zeros_like(x)
    for k in range(1, x.shape[1] - 1):
        a = x[:, k + 1] + x[:, k - 1] - 2 * x[:, k]
        b = (x[:, k + 1] - x[:, k - 1]) / 2
        out[:, k] = np.where(np.abs(b) >= np.abs(a), 0.0, -b / np.where(a == 0, 1.0, a))
    return out


def tables():
    thresholds = np.linspace(0, 1, 101)
    beta_probs = np.diff(scipy.stats.beta.cdf(thresholds, 2, 18))
    return thresholds, beta_probs


def observations(yin, shifts, c, sr=SR, fmin=FMIN):
    """6. Troughs, threshold priors, candidates -> observation probabilities [2*nb, F] and voiced_prob [F]."""
    thresholds, beta_probs = tables()
    nb = c["n_pitch_bins"]
    nf = yin.shape[0]
    probs_all = np.zeros_like(yin)
    for i in range(nf):
        x = yin[i]
        xp = np.pad(x, 1, mode="edge")
        is_trough = (x < xp[:-2]) & (x <= xp[2:])                  # localmin, edge padding
        is_trough[0] = x[0] < x[1]
        (ti,) = np.nonzero(is_trough)
        if len(ti) == 0:
            continue
        h = x[ti]
        below = np.less.outer(h, thresholds[1:])
        pos = np.cumsum(below, axis=0) - 1                         # rank in lag order among troughs below the threshold
        count = np.count_nonzero(below, axis=0)
        prior = scipy.stats.boltzmann.pmf(pos, 2, count)
        prior[~below] = 0
        probs = prior.dot(beta_probs)
        gm = np.argmin(h)                                          # first argmin
        n_below = np.count_nonzero(~below[gm, :])
        probs[gm] += 0.01 * np.sum(beta_probs[:n_below])
        probs_all[i, ti] = probs
    period, frame = np.nonzero(probs_all.T)                        # period-major: per frame, ascending lag
    cand = c["min_period"] + period + shifts[frame, period]
    f0c = sr / cand
    bins = 12 * c["bins_per_semitone"] * np.log2(f0c / fmin)
    bins = np.clip(np.round(bins), 0, nb).astype(int)              # half-to-even
    obs = np.zeros((2 * nb, nf))
    obs[bins, frame] = probs_all.T[period, frame]                  # last write (larger lag) wins; bin nb is overwritten below
    voiced = np.clip(np.sum(obs[:nb, :], axis=0, keepdims=True), 0, 1)   # sequential over rows
    obs[nb:, :] = (1 - voiced) / nb
    return obs, voiced[0]


def transition(c):
    """7. kron([[.99,.01],[.01,.99]], transition_local(nb, width, 'triangle', wrap=False)), dense, row-normalised."""
    nb, width = c["n_pitch_bins"], c["width"]
    w = scipy.signal.get_window("triangle", width, fftbins=False)
    T = np.zeros((nb, nb))
    for i in range(nb):
        row = np.zeros(nb)
        lp = (nb - width) // 2
        row[lp:lp + width] = w
        row = np.roll(row, nb // 2 + i + 1)
        row[min(nb, i + width // 2 + 1):] = 0
        row[:max(0, i - width // 2)] = 0
        T[i] = row
    T /= T.sum(axis=1, keepdims=True)
    return np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), T)


def log_obs(obs):
    return np.log(obs + TINY).T                                    # [F, 2*nb]


def viterbi(lobs, log_trans, log_p_init):
    """7. Dense Viterbi; argmax is the first index maximising the rounded fp64 sum.  lobs [F, S] -> states [F]."""
    nf, ns = lobs.shape
    value = lobs[0] + log_p_init
    ptr = np.zeros((nf, ns), dtype=np.int64)
    for t in range(1, nf):
        trans_out = value[:, None] + log_trans                     # [i, j]
        ptr[t] = np.argmax(trans_out, axis=0)
        value = lobs[t] + trans_out[ptr[t], np.arange(ns)]
    states = np.zeros(nf, dtype=np.int64)
    states[-1] = np.argmax(value)
    for t in range(nf - 2, -1, -1):
        states[t] = ptr[t + 1, states[t + 1]]
    return states


def viterbi_tables(c):
    nb = c["n_pitch_bins"]
    log_trans = np.log(transition(c) + TINY)
    p_init = np.zeros(2 * nb)
    p_init[nb:] = 1.0 / nb
    return log_trans, np.log(p_init + TINY)


def pyin(y, sr=SR, frame_length=FRAME, hop_length=HOP, pad=(FRAME - HOP) // 2, fmin=FMIN, fmax=FMAX, stages=False):
    """8. f0 float32 (0 where unvoiced), voiced flag, voiced_prob; with stages=True also the intermediate arrays."""
    c = consts(sr, frame_length, hop_length, fmin, fmax)
    fr = frames(y, pad, frame_length, hop_length)
    yin = cmndf(fr, c)
    sh = parabolic_shifts(yin)
    obs, vp = observations(yin, sh, c, sr, fmin)
    lo = log_obs(obs)
    lt, lpi = viterbi_tables(c)
    states = viterbi(lo, lt, lpi)
    nb = c["n_pitch_bins"]
    freqs = fmin * 2 ** (np.arange(nb) / (12 * c["bins_per_semitone"]))
    voiced = states < nb
    f0 = np.where(voiced, freqs[states % nb], 0.0).astype(np.float32)
    out = (f0, voiced, vp)
    if stages:
        out = out + (dict(cmndf=yin, shifts=sh, log_obs=lo, states=states, log_trans=lt, log_p_init=lpi),)
    return out
