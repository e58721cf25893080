"""GPU: pYIN pitch tracking (csrc/pyin.hip) against the float64 oracle (tests/pyin_f64.py) on a seeded synthetic corpus --
each stage fed the oracle's own inputs, then end to end; batch invariance, determinism and the dataset's cache-miss hook."""
import numpy as np
import pytest
import torch

import pyin_f64 as P

pytestmark = pytest.mark.gpu

SR = 16000


def _harmonic(f_inst, amp, rng, n_harm=5):
    phase = 2 * np.pi * np.cumsum(f_inst) / SR
    y = sum((0.6 ** k) * np.sin((k + 1) * phase + rng.uniform(0, 2 * np.pi)) for k in range(n_harm))
    return amp * y


def _corpus(seed=0):
    rng = np.random.default_rng(seed)
    t = lambda d: np.arange(int(d * SR)) / SR  # noqa: E731
    out = []
    # vowel with vibrato and jitter
    tt = t(1.0)
    f = 160 * (1 + 0.02 * np.sin(2 * np.pi * 5.5 * tt)) * (1 + 0.004 * rng.standard_normal(tt.size))
    out.append(_harmonic(f, 0.25, rng) + 0.003 * rng.standard_normal(tt.size))
    # glide 90 -> 700 Hz
    tt = t(0.8)
    out.append(_harmonic(90 * (700 / 90) ** (tt / tt[-1]), 0.3, rng))
    # jumps of more than 4.5 semitones with silence gaps
    segs = []
    for fq, d in ((220, 0.25), (330, 0.25), (0, 0.2), (140, 0.25), (520, 0.2)):
        n = int(d * SR)
        segs.append(np.zeros(n) if fq == 0 else _harmonic(np.full(n, float(fq)), 0.3, rng))
    out.append(np.concatenate(segs))
    # amplitude ramp down to the 1e-6 zeroing thresholds
    tt = t(0.6)
    out.append(_harmonic(np.full(tt.size, 250.0), 1.0, rng) * np.geomspace(0.3, 1e-5, tt.size))
    # white noise, the minimum length, a length between (repeated reflection) and 865 samples
    out.append(0.1 * rng.standard_normal(int(0.3 * SR)))
    out.append(_harmonic(np.full(320, 300.0), 0.3, rng))
    out.append(_harmonic(np.full(600, 200.0), 0.3, rng))
    out.append(_harmonic(np.full(865, 440.0), 0.3, rng))
    return [np.asarray(x, dtype=np.float32) for x in out]


@pytest.fixture(scope="module")
def corpus():
    wavs = _corpus()
    refs = [P.pyin(w, stages=True) for w in wavs]
    return wavs, refs


def _batch(wavs, dev):
    T = max(len(w) for w in wavs)
    y = torch.zeros(len(wavs), T)
    for i, w in enumerate(wavs):
        y[i, :len(w)] = torch.from_numpy(w)
    return y.to(dev), [len(w) for w in wavs]


def _lengths(ns, dev):
    from vcvits_amd.ops import pitch
    nfs = [pitch.pyin_n_frames(n) for n in ns]
    return (torch.tensor(ns, dtype=torch.int32, device=dev), torch.tensor(nfs, dtype=torch.int32, device=dev), nfs)


def _stack(arrs, F, tail):
    out = np.zeros((len(arrs), F) + tail)
    for i, a in enumerate(arrs):
        out[i, :len(a)] = a
    return out


def test_stage1_cmndf_and_shifts(gpu, corpus):
    from vcvits_amd import ops
    wavs, refs = corpus
    y, ns = _batch(wavs, gpu)
    n_samples, n_frames, nfs = _lengths(ns, gpu)
    cm, sh, bad = ops.pyin_yin(y, n_samples, n_frames, max(nfs))
    cm, sh = cm.cpu().numpy(), sh.cpu().numpy()
    worst = [0.0, 0.0]
    for i, (r, nf) in enumerate(zip(refs, nfs)):
        worst[0] = max(worst[0], float(np.abs(cm[i, :nf] - r[3]["cmndf"]).max()))
        worst[1] = max(worst[1], float(np.abs(sh[i, :nf] - r[3]["shifts"]).max()))
        assert not cm[i, nf:].any() and not sh[i, nf:].any()
    print("stage 1: largest |cmndf - oracle| %.3e, |shift - oracle| %.3e" % tuple(worst))
    assert worst[0] <= 1e-11 and worst[1] <= 1e-11, worst
    assert int(bad.item()) == 0


def test_stage2_log_observations(gpu, corpus):
    from vcvits_amd import ops
    wavs, refs = corpus
    nfs = [len(r[0]) for r in refs]
    F = max(nfs)
    cm = torch.from_numpy(_stack([r[3]["cmndf"] for r in refs], F, (239,))).to(gpu)
    sh = torch.from_numpy(_stack([r[3]["shifts"] for r in refs], F, (239,))).to(gpu)
    n_frames = torch.tensor(nfs, dtype=torch.int32, device=gpu)
    lobs, vp = ops.pyin_obs(cm, sh, n_frames)
    lobs, vp = lobs.cpu().numpy(), vp.cpu().numpy()
    L = np.log(P.TINY)
    worst, worst_u = 0.0, 0.0
    for i, (r, nf) in enumerate(zip(refs, nfs)):
        ref = r[3]["log_obs"]
        got = lobs[i, :nf]
        # the voiced block holds the candidates: identical support, values to 1e-12 relative
        assert np.array_equal(got[:, :601] == L, ref[:, :601] == L), "candidate support differs (row %d)" % i
        worst = max(worst, float((np.abs(got[:, :601] - ref[:, :601]) / np.abs(ref[:, :601])).max()))
        # the unvoiced fill is (1 - clip(sum of the candidates' probabilities, 0, 1)) / 601.  When the global minimum lies
        # below every threshold that sum is 1 up to rounding, and whether it lands on 1.0 (fill exactly 0, log(tiny)) or
        # one ulp below (fill ~1e-19, log ~ -43) follows the summation order of numpy's BLAS dot
        # (trough_prior.dot(beta_probs)), which depends on the CPU's BLAS kernel.  So the fill is compared as a
        # probability, and voiced_prob to 1e-12
        worst_u = max(worst_u, float(np.abs(np.exp(got[:, 601:]) - np.exp(ref[:, 601:])).max()))
        assert np.abs(vp[i, :nf] - r[2]).max() <= 1e-12
        assert not lobs[i, nf:].any() and not vp[i, nf:].any()
    print("stage 2: largest relative |log_obs - oracle| (voiced) %.3e, |unvoiced fill - oracle| %.3e" % (worst, worst_u))
    assert worst <= 1e-12 and worst_u <= 1e-17


def _viterbi_check(gpu, lobs_list):
    from vcvits_amd import ops
    lt, lpi = P.viterbi_tables(P.consts())
    nfs = [x.shape[0] for x in lobs_list]
    F = max(nfs)
    lo = torch.from_numpy(_stack(lobs_list, F, (1202,))).to(gpu)
    vp = torch.zeros(len(nfs), F, dtype=torch.float64, device=gpu)
    f0, voiced, _, cls, states = ops.pyin_viterbi(lo, vp, torch.tensor(nfs, dtype=torch.int32, device=gpu))
    states = states.cpu().numpy().astype(np.int64) & 0xFFFF
    for i, (x, nf) in enumerate(zip(lobs_list, nfs)):
        ref = P.viterbi(x, lt, lpi)
        assert np.array_equal(states[i, :nf], ref), "row %d: %d of %d states differ" % (i, int((states[i, :nf] != ref).sum()), nf)
        assert np.array_equal(voiced.cpu().numpy()[i, :nf], ref < 601)
    return states


def test_stage3_states_bit_identical(gpu, corpus):
    _, refs = corpus
    _viterbi_check(gpu, [r[3]["log_obs"] for r in refs])


def test_stage3_out_of_band_transitions_and_ties(gpu):
    L = float(np.log(P.TINY))
    rng = np.random.default_rng(5)
    cases = []
    cases.append(np.full((40, 1202), np.log(1 / 1202)))  # every state ties on every frame
    x = np.full((60, 1202), L)  # -708 runs with isolated far jumps: only out-of-band transitions reach them
    for t in range(60):
        x[t, rng.integers(0, 1202, size=2)] = np.log(rng.uniform(0.05, 0.9, size=2))
    cases.append(x)
    x = np.full((50, 1202), L)
    x[:, 601:] = np.log(1 / 601)  # unvoiced plateau, voiced spikes far apart (0 <-> 600) on alternate frames
    x[::2, 0] = np.log(0.9)
    x[1::2, 600] = np.log(0.9)
    cases.append(x)
    x = np.log(rng.uniform(0, 1, size=(45, 1202)) * (rng.uniform(size=(45, 1202)) < 0.02) + P.TINY)
    cases.append(x)
    _viterbi_check(gpu, cases)


def test_end_to_end_classes_match_the_oracle(gpu, corpus):
    from vcvits_amd import ops
    from vcvits_amd.data.audio import coarse_f0
    wavs, refs = corpus
    y, ns = _batch(wavs, gpu)
    f0, voiced, vp, cls, nf = ops.pyin(y, ns)
    f0, voiced, cls = f0.cpu(), voiced.cpu(), cls.cpu()
    for i, r in enumerate(refs):
        n = int(nf[i])
        assert np.array_equal(f0[i, :n].numpy(), r[0]), "row %d f0" % i
        assert np.array_equal(voiced[i, :n].numpy(), r[1]), "row %d voicing" % i
        assert torch.equal(cls[i, :n], coarse_f0(torch.from_numpy(r[0]))), "row %d classes" % i
        assert not cls[i, n:].any()


def test_batch_invariance_and_determinism(gpu, corpus):
    from vcvits_amd import ops
    wavs, _ = corpus
    y, ns = _batch(wavs, gpu)
    full = [t.cpu() for t in ops.pyin(y, ns)[:4]]
    again = [t.cpu() for t in ops.pyin(y, ns)[:4]]
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for i, w in enumerate(wavs):
        one = ops.pyin(torch.from_numpy(w).to(gpu).unsqueeze(0))
        n = int(one[4][0])
        for a, b in zip(full, one[:4]):
            assert torch.equal(a[i, :n], b[0].cpu()), "row %d differs from its single run" % i


def test_estimate_pitch_and_pitch_classes(gpu, corpus):
    from vits.data.audio import coarse_f0, estimate_pitch, pitch_classes
    wavs, refs = corpus
    p = estimate_pitch(wavs[0], 16000, 2048, 2048, 320)
    assert p.device.type == "cpu" and p.dtype == torch.float32 and p.shape == (1, len(refs[0][0]))
    assert np.array_equal(p[0].numpy(), refs[0][0])
    pd = estimate_pitch(torch.from_numpy(wavs[0]).to(gpu), 16000, 2048, 2048, 320)
    assert pd.is_cuda and torch.equal(pd.cpu(), p)
    y, ns = _batch(wavs, gpu)
    cls, nf = pitch_classes(y, ns, 16000, 2048, 2048, 320, f0_bin=512)
    for i, w in enumerate(wavs):
        want = coarse_f0(estimate_pitch(w, 16000, 2048, 2048, 320), f0_bin=512)
        assert torch.equal(cls[i:i + 1, :int(nf[i])].cpu(), want)
    bad = torch.from_numpy(wavs[0].copy())
    bad[100] = float("nan")
    with pytest.raises(ValueError):
        estimate_pitch(bad.to(gpu), 16000, 2048, 2048, 320)


def test_dataset_cache_miss_round_trip(gpu, corpus, tmp_path):
    import types
    from vits.data.audio import coarse_f0, estimate_pitch
    from vcvits_amd.data.dataset import VoiceConversionMultiSpeakerDataset, cache_paths
    wavs, refs = corpus
    hp = types.SimpleNamespace(source_sampling_rate=16000, target_sampling_rate=22050, filter_length=2048, hop_length=256,
                               win_length=2048, num_pitch=512)
    audio = {"a.wav": wavs[0], "b.wav": wavs[2]}
    calls = []

    def load_audio(path, sr):
        return torch.from_numpy(audio[path].copy())

    def get_pitch(path, filter_length, win_length, num_pitch, sr):
        calls.append(path)
        return coarse_f0(estimate_pitch(load_audio(path, sr).numpy(), sr, filter_length, win_length, 320), f0_bin=num_pitch)

    ds = VoiceConversionMultiSpeakerDataset([["a.wav", "0"], ["b.wav", "1"]], hp, str(tmp_path), load_audio=load_audio,
                                            get_pitch=get_pitch)
    first = [ds[i]["x_pitch"] for i in range(2)]
    assert len(calls) == 2
    for i in range(2):
        path = ds.audiopaths[i][0]
        stored = torch.load(cache_paths(str(tmp_path), path, hp)[1])
        assert torch.equal(stored, first[i])
        ref = refs[0] if path == "a.wav" else refs[2]
        assert torch.equal(first[i], coarse_f0(torch.from_numpy(ref[0]).unsqueeze(0), f0_bin=512))
    second = [ds[i]["x_pitch"] for i in range(2)]
    assert len(calls) == 2 and all(torch.equal(a, b) for a, b in zip(first, second))
