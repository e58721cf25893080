"""pYIN pitch tracking (csrc/pyin.hip): librosa.pyin as the reference's estimate_pitch calls it (vits/data/audio.py:24-63),
batched over utterances of different lengths.

Part of `vcvits_amd.ops` (the package re-exports every name: `from vcvits_amd import ops; ops.pyin(...)`).  The host builds
the tables whose values must match numpy / scipy to the last bit (thresholds, beta and Boltzmann probabilities, the
log-transition band, bin frequencies, the pitch-class table) once per device and parameters; every launch goes to
libvcvits_hip.so on the current stream.  There is no CPU fallback: CPU tensors raise."""
import numpy as np
import torch

from .._lib import check, lib, ptr, stream

PYIN_TINY = float(np.finfo(np.float64).tiny)
PYIN_LOG_TINY = float(np.log(PYIN_TINY))  # what every zero probability becomes: log(0 + tiny)
PYIN_FMIN = 440.0 * 2.0 ** ((36 - 69) / 12.0)  # librosa.note_to_hz('C2')
PYIN_FMAX = 440.0 * 2.0 ** ((96 - 69) / 12.0)  # librosa.note_to_hz('C7')
PYIN_PMF_LD = 128  # Boltzmann table [count, rank]; at most 120 troughs in 239 lags
_PYIN_FRAME = 2048  # the kernels' LDS layout
_pyin_host = {}
_pyin_dev = {}


def pyin_consts(sr=16000, frame_length=2048, hop_length=320, fmin=PYIN_FMIN, fmax=PYIN_FMAX):
    """librosa.pyin's derived constants (win_length = frame_length // 2, resolution 0.1, max_transition_rate 35.92)."""
    win = frame_length // 2
    min_period = max(int(np.floor(sr / fmax)), 1)
    max_period = min(int(np.ceil(sr / fmin)), frame_length - win - 1)
    per_semitone = int(np.ceil(1.0 / 0.1))
    n_bins = int(np.floor(12 * per_semitone * np.log2(fmax / fmin))) + 1
    width = round(35.92 * 12 * hop_length / sr) * per_semitone + 1
    return {"win_length": win, "min_period": min_period, "max_period": max_period, "n_lags": max_period - min_period + 1,
            "bins_per_semitone": per_semitone, "n_bins": n_bins, "n_states": 2 * n_bins, "transition_width": width}


def pyin_n_frames(n, frame_length=2048, hop_length=320, pad=864):
    """Frames of an utterance of n samples after reflect padding by `pad` (center=False framing)."""
    return 1 + (n + 2 * pad - frame_length) // hop_length


def _pyin_check_consts(c, frame_length):
    if frame_length != _PYIN_FRAME:
        raise NotImplementedError("pyin kernels: frame_length (= win_length) 2048 only (both reference configs)")
    if c["n_bins"] != 601 or c["transition_width"] != 91 or c["n_lags"] > 256 or c["n_lags"] < 3:
        raise NotImplementedError("pyin kernels: 601 pitch bins, a 91-bin transition band and < 256 lags "
                                  "(sr 16000, hop 320, fmin C2, fmax C7: the reference's parameters); got %s" % (c,))


def _pyin_dense_transition(n, width):
    """librosa.sequence.transition_local(n, width, window='triangle', wrap=False): dense, row-normalised by numpy."""
    import scipy.signal
    w = scipy.signal.get_window("triangle", width, fftbins=False)
    T = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        row = np.zeros(n)
        left = (n - width) // 2
        row[left:left + width] = w
        row = np.roll(row, n // 2 + i + 1)
        row[min(n, i + width // 2 + 1):] = 0
        row[:max(0, i - width // 2)] = 0
        T[i] = row
    T /= T.sum(axis=1, keepdims=True)
    return T


def pyin_host_tables(sr=16000, frame_length=2048, hop_length=320, fmin=PYIN_FMIN, fmax=PYIN_FMAX, f0_bin=512):
    """The numpy-exact tables of the three kernels (cached per parameters), as numpy arrays."""
    key = (sr, frame_length, hop_length, float(fmin), float(fmax), f0_bin)
    if key in _pyin_host:
        return _pyin_host[key]
    import scipy.stats
    c = pyin_consts(sr, frame_length, hop_length, fmin, fmax)
    _pyin_check_consts(c, frame_length)
    nb, width = c["n_bins"], c["transition_width"]
    half = width // 2
    thresholds = np.linspace(0, 1, 101)
    beta_probs = np.diff(scipy.stats.beta.cdf(thresholds, 2, 18))
    gm_bonus = np.array([0.01 * np.sum(beta_probs[:n]) for n in range(101)])
    counts = np.arange(PYIN_PMF_LD)[:, None]
    ranks = np.arange(PYIN_PMF_LD)[None, :]
    valid = (ranks < counts) & (counts > 0)
    with np.errstate(all="ignore"):
        pmf = scipy.stats.boltzmann.pmf(np.where(valid, ranks, 0), 2, np.maximum(counts, 1))
    pmf = np.where(valid, pmf, 0.0)
    # 7. log(kron([[.99, .01], [.01, .99]], T) + tiny) from numpy's dense matrix: the rows of T are NOT shifted copies
    # of each other (their pairwise row sums differ in the last bits), so every band entry is read from it
    lt = np.log(np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), _pyin_dense_transition(nb, width)) + PYIN_TINY)
    assert np.array_equal(lt[:nb, :nb], lt[nb:, nb:]) and np.array_equal(lt[:nb, nb:], lt[nb:, :nb])
    i, j = np.indices((nb, nb))
    inband = np.abs(i - j) <= half
    for blk in (lt[:nb, :nb], lt[nb:, :nb]):
        assert np.all(blk[~inband] == PYIN_LOG_TINY), "an out-of-band transition is not log(tiny)"
        assert np.all(blk[inband] > PYIN_LOG_TINY)
    # band[s][d][t] = log-transition into bin t from bin t + d - half of the same (s = 0) / the other (s = 1) block
    band = np.full((2, width, nb), PYIN_LOG_TINY)
    t = np.arange(nb)
    for d in range(width):
        src = t + d - half
        ok = (src >= 0) & (src < nb)
        band[0, d, ok] = lt[src[ok], t[ok]]
        band[1, d, ok] = lt[nb + src[ok], t[ok]]
    p_init = np.zeros(2 * nb)
    p_init[nb:] = 1.0 / nb
    log_p_init = np.log(p_init + PYIN_TINY)
    # 8. f0 = float32(fmin * 2 ** (bin / 120)), 0 unvoiced (index nb); classes from the product's own CPU coarse_f0
    from ..data.audio import coarse_f0
    freqs = fmin * 2 ** (np.arange(nb) / (12 * c["bins_per_semitone"]))
    f0_table = np.concatenate([freqs, [0.0]]).astype(np.float32)
    class_table = coarse_f0(torch.from_numpy(f0_table.copy()), f0_bin=f0_bin).numpy().astype(np.float32)
    tabs = {"consts": c, "thresholds": thresholds, "beta_probs": beta_probs, "gm_bonus": gm_bonus, "pmf": pmf,
            "band": band, "log_p_init": log_p_init, "f0_table": f0_table, "class_table": class_table}
    _pyin_host[key] = tabs
    return tabs


def pyin_tables(device, sr=16000, frame_length=2048, hop_length=320, fmin=PYIN_FMIN, fmax=PYIN_FMAX, f0_bin=512):
    """pyin_host_tables on `device` (cached per device and parameters)."""
    key = (str(device), sr, frame_length, hop_length, float(fmin), float(fmax), f0_bin)
    if key not in _pyin_dev:
        h = pyin_host_tables(sr, frame_length, hop_length, fmin, fmax, f0_bin)
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in h.items() if k != "consts"}
        dev["consts"] = h["consts"]
        _pyin_dev[key] = dev
    return _pyin_dev[key]


def _pyin_gpu(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("vcvits_amd: %s is not on the GPU; the HIP path has no CPU fallback" % what)
    return t.contiguous()


def pyin_yin(y, n_samples, n_frames, Fmax, *, hop_length=320, pad=864, sr=16000, fmin=PYIN_FMIN, fmax=PYIN_FMAX,
             frame_length=2048):
    """Stage 1 (contract 1.-5.): y [B, T] float32, n_samples / n_frames int32 [B] on the device ->
    (cmndf [B, Fmax, n_lags] fp64, shifts [B, Fmax, n_lags] fp64, nonfinite int32 [1])."""
    y = _pyin_gpu(y, "y")
    if y.dtype != torch.float32 or y.dim() != 2:
        raise RuntimeError("pyin: y must be float32 [B, T]")
    c = pyin_consts(sr, frame_length, hop_length, fmin, fmax)
    _pyin_check_consts(c, frame_length)
    B, T = y.shape
    cm = torch.empty((B, Fmax, c["n_lags"]), dtype=torch.float64, device=y.device)
    sh = torch.empty_like(cm)
    bad = torch.zeros((1,), dtype=torch.int32, device=y.device)
    check(lib().vcv_pyin_yin(ptr(y), ptr(_pyin_gpu(n_samples, "n_samples")), ptr(_pyin_gpu(n_frames, "n_frames")), B, T,
                             Fmax, frame_length, hop_length, pad, c["min_period"], c["max_period"], PYIN_TINY, ptr(cm),
                             ptr(sh), ptr(bad), stream()), "vcv_pyin_yin")
    return cm, sh, bad


def pyin_obs(cmndf, shifts, n_frames, *, sr=16000, frame_length=2048, hop_length=320, fmin=PYIN_FMIN, fmax=PYIN_FMAX):
    """Stage 2 (contract 6.): cmndf / shifts [B, F, n_lags] fp64 -> (log_obs [B, F, 1202] fp64, voiced_prob [B, F] fp64)."""
    cmndf, shifts = _pyin_gpu(cmndf, "cmndf"), _pyin_gpu(shifts, "shifts")
    tb = pyin_tables(cmndf.device, sr, frame_length, hop_length, fmin, fmax)
    c = tb["consts"]
    B, F, L = cmndf.shape
    if L != c["n_lags"] or cmndf.dtype != torch.float64 or shifts.shape != cmndf.shape or shifts.dtype != torch.float64:
        raise RuntimeError("pyin_obs: cmndf / shifts must be float64 [B, F, %d]" % c["n_lags"])
    lobs = torch.empty((B, F, c["n_states"]), dtype=torch.float64, device=cmndf.device)
    vp = torch.empty((B, F), dtype=torch.float64, device=cmndf.device)
    check(lib().vcv_pyin_obs(ptr(cmndf), ptr(shifts), ptr(_pyin_gpu(n_frames, "n_frames")), B, F, L, c["min_period"],
                             ptr(tb["thresholds"]), ptr(tb["beta_probs"]), ptr(tb["gm_bonus"]), ptr(tb["pmf"]),
                             PYIN_PMF_LD, float(sr), float(fmin), PYIN_TINY, PYIN_LOG_TINY, ptr(lobs), ptr(vp), stream()),
          "vcv_pyin_obs")
    return lobs, vp


def pyin_viterbi(log_obs, voiced_prob, n_frames, *, sr=16000, frame_length=2048, hop_length=320, fmin=PYIN_FMIN,
                 fmax=PYIN_FMAX, f0_bin=512):
    """Stage 3 (contract 7.-8.): log_obs [B, F, 1202] fp64, voiced_prob [B, F] fp64 ->
    (f0 float32, voiced bool, voiced_prob float32, pitch class float32, states int16), each [B, F]."""
    log_obs, voiced_prob = _pyin_gpu(log_obs, "log_obs"), _pyin_gpu(voiced_prob, "voiced_prob")
    tb = pyin_tables(log_obs.device, sr, frame_length, hop_length, fmin, fmax, f0_bin)
    c = tb["consts"]
    B, F, S = log_obs.shape
    if S != c["n_states"] or log_obs.dtype != torch.float64 or tuple(voiced_prob.shape) != (B, F) or \
            voiced_prob.dtype != torch.float64:
        raise RuntimeError("pyin_viterbi: log_obs float64 [B, F, %d] and voiced_prob float64 [B, F] expected" % c["n_states"])
    dev = log_obs.device
    bp = torch.empty((B, F, S), dtype=torch.int16, device=dev)
    f0 = torch.empty((B, F), dtype=torch.float32, device=dev)
    voiced = torch.empty((B, F), dtype=torch.uint8, device=dev)
    vpf = torch.empty((B, F), dtype=torch.float32, device=dev)
    cls = torch.empty((B, F), dtype=torch.float32, device=dev)
    states = torch.empty((B, F), dtype=torch.int16, device=dev)
    check(lib().vcv_pyin_viterbi(ptr(log_obs), ptr(voiced_prob), ptr(_pyin_gpu(n_frames, "n_frames")), B, F, S,
                                 ptr(tb["log_p_init"]), ptr(tb["band"]), c["transition_width"], PYIN_LOG_TINY,
                                 ptr(tb["f0_table"]), ptr(tb["class_table"]), ptr(bp), ptr(f0), ptr(voiced), ptr(vpf),
                                 ptr(cls), ptr(states), stream()), "vcv_pyin_viterbi")
    return f0, voiced.view(torch.bool), vpf, cls, states


def pyin_lengths(lengths, B, T, frame_length=2048, hop_length=320, pad=864):
    """Host-side checks of the utterance lengths -> (n_samples list, n_frames list).  librosa's rule: an utterance
    shorter than one frame after padding raises ValueError."""
    if lengths is None:
        ns = [int(T)] * B
    else:
        ns = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(ns) != B:
        raise ValueError("pyin: %d lengths for %d rows" % (len(ns), B))
    for n in ns:
        if n > T or n < 2 or n + 2 * pad < frame_length:
            raise ValueError("pyin: an utterance of %d samples (padded by %d per side) is shorter than frame_length=%d "
                             "or longer than its row (%d)" % (n, pad, frame_length, T))
    return ns, [pyin_n_frames(n, frame_length, hop_length, pad) for n in ns]


def pyin(y, lengths=None, *, sr=16000, frame_length=2048, hop_length=320, pad=None, fmin=PYIN_FMIN, fmax=PYIN_FMAX,
         f0_bin=512, check_finite=True):
    """librosa.pyin(frame_length, hop_length, fmin, fmax, center=False) of each row of y [B, T] float32 (device), reflect-
    padded by `pad` (default (frame_length - hop_length) // 2, as estimate_pitch pads) at its own length (`lengths`,
    default T).  Returns (f0, voiced_flag, voiced_prob, pitch_class, n_frames): [B, Fmax] float32 (0 where unvoiced),
    bool, float32, float32 whole numbers (coarse_f0(f0, f0_bin)), and the frames of each row (CPU int64 [B]); frames past a
    row's own count are 0.  check_finite: read the kernel's non-finite flag (one device synchronisation) and raise
    ValueError as librosa does."""
    y = _pyin_gpu(y, "y")
    if y.dim() == 1:
        y = y.unsqueeze(0)
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError("pyin: y must be float32 [B, T] or [T]")
    pad = (frame_length - hop_length) // 2 if pad is None else int(pad)
    B, T = y.shape
    ns, nfs = pyin_lengths(lengths, B, T, frame_length, hop_length, pad)
    Fmax = max(nfs)
    dev = y.device
    n_samples = torch.tensor(ns, dtype=torch.int32).to(dev, non_blocking=True)
    n_frames = torch.tensor(nfs, dtype=torch.int32).to(dev, non_blocking=True)
    kw = dict(sr=sr, frame_length=frame_length, hop_length=hop_length, fmin=fmin, fmax=fmax)
    pyin_tables(dev, f0_bin=f0_bin, **kw)
    cm, sh, bad = pyin_yin(y, n_samples, n_frames, Fmax, pad=pad, **kw)
    lobs, vp = pyin_obs(cm, sh, n_frames, **kw)
    f0, voiced, vpf, cls, _ = pyin_viterbi(lobs, vp, n_frames, f0_bin=f0_bin, **kw)
    if check_finite and int(bad.item()):
        raise ValueError("pyin: audio buffer is not finite everywhere")
    return f0, voiced, vpf, cls, torch.tensor(nfs, dtype=torch.int64)
