"""The host planners of the packed-weight conv families, pinned: for a census of launch shapes, what each family answers
(return code, the three `_plan` words, the `_pack_job` fields, the sixteen `vcv_conv_plan_describe` words) under the default
switches, under every planner switch and under the forced split-operand variants.  The planners are host-only: no GPU.

tests/golden/conv_plan_census.npz holds the answers of the planners as they were BEFORE their shared skeleton
(csrc/conv_plan.h) existed; `python tests/test_conv_plan_census.py --record` rewrites it from the library that is built."""
import ctypes
import hashlib
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from vcvits_amd import configs, tuning  # noqa: E402
from vcvits_amd._lib import TF_LEAKY, TF_NONE, VcvConvArgs, VcvPackJob, lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan_census.npz")
FAMILIES = ("dma", "pk", "bf16", "x3", "bf16io")  # the `family` argument of vcv_conv_plan_describe, in order
PLAN = ("vcv_conv_dma_plan", "vcv_conv_pk_plan", "vcv_conv_bf16_plan", "vcv_conv_x3_plan", "vcv_conv_bf16io_plan")
PACK_JOB = (None, "vcv_conv_pk_pack_job", "vcv_conv_bf16_pack_job", "vcv_conv_x3_pack_job", None)
JOB_FIELDS = ("kind", "M", "C", "K", "BM", "BKC", "JA", "nch", "nmt", "phases", "mode", "total")
NW = 1 + 1 + 3 + len(JOB_FIELDS) + 16  # plan rc, describe rc, plan words, job fields, describe words
SWITCHES = [("default", None, None)] + [(k + "=%d" % v, k, v) for k, v in (
    ("x3_all", 1), ("x3_merge_phases", 0), ("x3_js2", 0), ("x3_v6", 0), ("x3_old_ks", 1), ("pk_x4", 0), ("pk_ws", 0), ("pk_vec", 0),
    ("xcd_remap", 0))] + [("x3_variant=%d" % v, "x3_variant", v) for v in range(7)]
EXPLICIT_EVERY = 400  # the explicit grid keeps one combination in so many, the hashed one one in 4 (a multiple of 4: see grid_rows)
PTR = 0x10000  # a stand-in for "this operand is given": the planners look at pointers' presence and alignment only


def _args(B, Cg, Mg, Tin, Tout, P, K, s, dj, off, os_=1, oo=0, phases=1, Q=None, a_mode=0, leaky=0, res=0, mask=0, oaux=0,
          accumulate=0, io=0, ms=0, post_scale=0.0, y=PTR, G=1, slope=0.1, flip=0):
    a = VcvConvArgs()
    a.B, a.G, a.Cg, a.Mg, a.Tin, a.Tout, a.P, a.K = B, G, Cg, Mg, Tin, Tout, P, K
    a.s, a.dj, a.off, a.os, a.oo, a.phases, a.Q, a.a_mode = s, dj, off, os_, oo, phases, Tout if Q is None else Q, a_mode
    a.in_tf, a.accumulate, a.alpha, a.slope = TF_LEAKY if leaky else TF_NONE, accumulate, 1.0, slope
    a.io, a.ms, a.post_scale = io, ms, post_scale
    a.x, a.w, a.y = PTR, PTR, y
    a.res, a.mask, a.oaux = (PTR if res else None), (PTR if mask else None), (PTR if oaux else None)
    return a, flip


def _out_len(tin, k, s, pad, dil):
    return (tin + 2 * pad - dil * (k - 1) - 1) // s + 1


# the launches ops/conv.py and ops/x16.py build for one layer (same fields, same arithmetic)
def forward(B, C, M, T, K, s=1, dil=1, P=1, pad=None, **kw):
    pad = dil * (K - 1) // 2 if pad is None else pad
    return _args(B, C, M, T, _out_len(T, K, s, pad, dil), P, K, s, dil, -pad, **kw)


def dgrad(B, C, M, T, K, s=1, dil=1, P=1, pad=None, **kw):
    """Data gradient of forward(): the flipped stride-1 form, the a_mode 1 stride-1 form (narrow layers), or the phased one."""
    pad = dil * (K - 1) // 2 if pad is None else pad
    Tout = _out_len(T, K, s, pad, dil)
    if s == 1 and M >= 32 and C >= 32:
        return _args(B, M, C, Tout, T, P, K, 1, dil, pad - (K - 1) * dil, Q=T, flip=1, **kw)
    if s == 1:
        return _args(B, M, C, Tout, T, P, K, 1, -dil, pad, Q=T, a_mode=1, **kw)
    return _args(B, M, C, Tout, T, P, K, 1, -1, 0, s, -pad, s, (T - 1 + pad) // s + 1, 1, **kw)


def convT(B, C, M, T, K, s, pad=None, merged=False, **kw):
    pad = (K - s) // 2 if pad is None else pad
    Tout = (T - 1) * s - 2 * pad + K
    if s == 1:
        return _args(B, C, M, T, Tout, 1, K, 1, -1, pad, a_mode=1, **kw)
    Q = (Tout - 1 + pad) // s + 1
    if merged:
        return _args(B, C, M * s, T, Tout, 1, K // s, 1, -1, 0, s, -pad, 1, Q, 1, ms=s, **kw)
    return _args(B, C, M, T, Tout, 1, K, 1, -1, 0, s, -pad, s, Q, 1, **kw)


def convT_dgrad(B, C, M, T, K, s, pad=None, **kw):
    pad = (K - s) // 2 if pad is None else pad
    return _args(B, M, C, (T - 1) * s - 2 * pad + K, T, 1, K, s, 1, -pad, Q=T, **kw)


def layer_rows():
    """Every GEMM-shaped conv launch of configs.base() / base_48k(): training (segment of 32 frames, the batches of the
    benchmark's legs), and the 938-frame decode with 16-bit activations."""
    rows = []
    for cfg, batches in ((configs.base(), (16, 32)), (configs.base_48k(), (16,))):
        m = cfg["model"]
        H, up0 = m["hidden_channels"], m["upsample_initial_channel"]
        frames = cfg["train"]["segment_size"] // cfg["data"]["hop_length"]
        for B in batches:
            # generator: conv_pre, the transposed stages, the ResBlock convs of every stage
            rows += [forward(B, m["inter_channels"], up0, frames, 7), dgrad(B, m["inter_channels"], up0, frames, 7)]
            T, ch = frames, up0
            for r, k in zip(m["upsample_rates"], m["upsample_kernel_sizes"]):
                rows += [convT(B, ch, ch // 2, T, k, r, leaky=1), convT_dgrad(B, ch, ch // 2, T, k, r, oaux=1)]
                if T <= 64:  # (the batch folded into the columns: ops/conv.py, _ConvFn)
                    rows += [convT(1, ch, ch // 2, T, k, r, leaky=1)]
                T, ch = T * r, ch // 2
                for rk, dils in zip(m["resblock_kernel_sizes"], m["resblock_dilation_sizes"]):
                    for d in dils:
                        rows += [forward(B, ch, ch, T, rk, dil=d, leaky=1), forward(B, ch, ch, T, rk, leaky=1, res=1),
                                 dgrad(B, ch, ch, T, rk, dil=d, oaux=1), dgrad(B, ch, ch, T, rk, oaux=1, res=1)]
            # period discriminators (real and generated stacked: 2 B), the last convs of DiscriminatorS
            seg = cfg["train"]["segment_size"]
            for p in m.get("multi_period_discriminator_periods", [2, 3, 5, 7, 11, 17, 23, 37]):
                Hh = _out_len(-(-seg // p), 5, 3, 2, 1)  # (after the 1 -> 32 conv)
                for C, M, s in ((32, 128, 3), (128, 512, 3), (512, 1024, 3), (1024, 1024, 1)):
                    rows += [forward(2 * B, C, M, Hh, 5, s, P=p, pad=2), dgrad(2 * B, C, M, Hh, 5, s, P=p, pad=2, oaux=1),
                             dgrad(B, C, M, Hh, 5, s, P=p, pad=2, oaux=1)]
                    Hh = _out_len(Hh, 5, s, 2, 1)
            rows += [forward(1, 1024, 1024, T_, 5, P=2 * B) for T_ in (64, 16)] + [dgrad(1, 1024, 1024, 64, 5, P=2 * B)]
            # posterior encoder / flow WaveNets, text-side attention and FFN projections (masked)
            for T_ in (frames, 400):
                rows += [forward(B, H, 2 * H, T_, 5), dgrad(B, H, 2 * H, T_, 5), forward(B, H, 2 * H, T_, 1, mask=1),
                         dgrad(B, H, 2 * H, T_, 1), forward(B, H, H, T_, 1), forward(B, H, m["filter_channels"], T_, 3, mask=1),
                         dgrad(B, H, m["filter_channels"], T_, 3, mask=1), forward(B, m["filter_channels"], H, T_, 3, mask=1),
                         forward(B, m["hubert_channels"], H, T_, 1), forward(B, cfg["data"]["n_mel_channels"], H, T_, 1)]
    # the 64 x 938-frame decode of the 48 kHz config: fp32 and every 16-bit storage combination
    m = configs.base_48k()["model"]
    T, ch = 938, m["upsample_initial_channel"]
    for r, k in zip(m["upsample_rates"], m["upsample_kernel_sizes"]):
        rows += [convT(64, ch, ch // 2, T, k, r, leaky=1), convT(64, ch, ch // 2, T, k, r, leaky=1, io=15),
                 convT(64, ch, ch // 2, T, k, r, leaky=1, io=15, merged=True)]
        T, ch = T * r, ch // 2
        for rk, dils in zip(m["resblock_kernel_sizes"], m["resblock_dilation_sizes"]):
            for d in dils:
                rows += [forward(64, ch, ch, T, rk, dil=d, leaky=1), forward(64, ch, ch, T, rk, dil=d, leaky=1, io=7),
                         forward(64, ch, ch, T, rk, leaky=1, res=1, io=11),
                         forward(64, ch, ch, T, rk, leaky=1, res=1, io=11, accumulate=1, post_scale=1 / 3)]
    return rows


def grid_rows(dense):
    """A grid over B, Cg, Mg, T, K, s, dil and P.  Mg straddles 48, 64, 96, 128 and 256; the row lengths put U = Q * P into
    the 160-224 and 256-288 bands and either side of them; P > 1; phased launches of 2, 3 and 4 residues; io = 15 with ms > 1."""
    Bs = (1, 2, 16, 64)
    Cs = (16, 24, 32, 64, 96, 130, 256, 1024)
    Ms = (31, 32, 47, 48, 63, 64, 65, 95, 96, 127, 128, 129, 255, 256, 257, 512, 1024)
    Ts = (40, 95, 96, 128, 160, 161, 200, 224, 225, 256, 257, 280, 288, 289, 320, 330, 620, 1300, 2048, 8192, 11777)
    Ks = (1, 2, 3, 4, 5, 7, 11, 16, 17)
    rows = []
    for n, (B, C, M, T, K) in enumerate(itertools.product(Bs, Cs, Ms, Ts, Ks)):
        h = (n * 2654435761 >> 7) & 0xffff  # (deterministic variety instead of a product over every flag)
        if (h >> 4) % (4 if dense else EXPLICIT_EVERY) != 0:
            continue  # the explicit grid is a subset of the hashed one
        kw = dict(leaky=h & 1, res=(h >> 1) & 1, mask=(h >> 2) & 1)
        rows.append(forward(B, C, M, T, K, dil=(1, 3, 5, 1)[h & 3], **kw))
        rows.append(dgrad(B, C, M, T, K, oaux=h & 1))
        P = (2, 3, 5, 7)[h & 3]
        rows.append(forward(B, C, M, -(-T // P), K, (1, 2, 3, 4)[(h >> 2) & 3], P=P, **kw))
        rows.append(dgrad(B, C, M, -(-T // P), K, (2, 3, 3, 4)[(h >> 2) & 3], P=P, oaux=h & 1))
        s = (2, 4, 8, 3)[(h >> 2) & 3]
        Kt = max(K, s) if h & 8 else -(-K // s) * s
        rows.append(convT(B, C, M, T // 4, Kt, s, leaky=1))
        io = (3, 7, 11, 15)[h & 3]
        rows.append(forward(B, C, M, T & ~1, K, io=io, y=PTR + (8 if h & 48 == 16 else 0), **kw))
        rows.append(convT(B, C, M, T // 4, Kt, s, leaky=1, io=15, merged=Kt % s == 0))
    return rows


def answers(rows, families=range(5), hashed=False):
    """int64 [family, row, NW].  hashed (the large grid): a family is asked about the rows of its own storage type only, and
    vcv_conv_plan_describe only where its _plan accepts -- the explicit rows ask every family everything."""
    L = lib()
    out = []
    plan, desc, job = (ctypes.c_int64 * 3)(), (ctypes.c_int32 * 16)(), VcvPackJob()
    declined = [0] * (NW - 2)
    for f in range(5):
        plan_fn, job_fn, describe = getattr(L, PLAN[f]), (getattr(L, PACK_JOB[f]) if PACK_JOB[f] else None), L.vcv_conv_plan_describe
        words = []
        for a, flip in rows if f in families else ():
            if hashed and (a.io != 0) != (f == 4):
                continue
            ref = ctypes.byref(a)
            rc = plan_fn(ref, flip, plan)
            if rc != 0:
                words += [rc, rc if hashed else describe(ref, f, flip, desc)] + declined
                continue
            words += [rc, describe(ref, f, flip, desc)] + plan[:]
            if job_fn is not None and job_fn(ref, flip, ctypes.byref(job)) == 0:
                words += [job.kind, job.M, job.C, job.K, job.BM, job.BKC, job.JA, job.nch, job.nmt, job.phases, job.mode, job.total]
            else:
                words += declined[:len(JOB_FIELDS)]
            words += desc[:]
        out.append(np.array(words, dtype=np.int64).reshape(-1, NW))
    return out if hashed else np.stack([o if len(o) else np.zeros((len(rows), NW), dtype=np.int64) for o in out])


class switched:
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        if self.key is not None:
            self.old = tuning.kernel_get(self.key)
            tuning.kernel_set(self.key, self.value)

    def __exit__(self, *exc):
        if self.key is not None:
            tuning.kernel_set(self.key, self.old)


def explicit_rows():
    seen, rows = set(), []
    for a, flip in layer_rows() + grid_rows(dense=False):
        if (bytes(a), flip) not in seen:
            seen.add((bytes(a), flip))
            rows.append((a, flip))
    return rows


def census():
    explicit = explicit_rows()
    got = {"explicit/" + name: None for name, _, _ in SWITCHES}
    for name, key, value in SWITCHES:
        with switched(key, value):
            # (the x3 switches reach the split-operand planner alone)
            got["explicit/" + name] = answers(explicit, (3,) if key is not None and key.startswith("x3") else range(5))
    dense = answers(grid_rows(dense=True), hashed=True)
    for f, fam in enumerate(FAMILIES):
        got["sha256/" + fam] = np.frombuffer(hashlib.sha256(dense[f].tobytes()).digest(), dtype=np.uint8)
    got["hashed_rows"] = np.array([[len(d), int((d[:, 0] == 0).sum())] for d in dense])  # asked, accepted
    return got


@pytest.fixture(scope="module")
def got():
    return census()


def test_census_is_not_vacuous(got):
    a = got["explicit/default"]
    for f, fam in enumerate(FAMILIES):
        taken = int((a[f, :, 0] == 0).sum())
        assert 0 < taken < a.shape[1], "%s: %d of %d rows accepted" % (fam, taken, a.shape[1])
        assert (a[f, :, 0] == a[f, :, 1]).all(), "%s: vcv_conv_plan_describe and %s disagree on a return code" % (fam, PLAN[f])
    d = a[:, :, -16:]
    assert (d[3, :, 14] == 1).any() and (d[4, :, 14] == 1).any(), "no merged-phase launch in the census"
    assert (d[:, :, 8] > 1).any(axis=1)[[0, 1, 2, 3]].all(), "a family never split its reduction"
    P_gt_1 = np.array([r[0].P > 1 for r in explicit_rows()])
    assert (a[:4, P_gt_1, 0] == 0).any(axis=1).all(), "no accepted period-layout row"
    for key in ("x3_all=1", "x3_merge_phases=0", "x3_js2=0", "x3_v6=0", "x3_old_ks=1"):
        assert (got["explicit/" + key][3] != a[3]).any(), "%s changes no plan of the census" % key
    for key, fams in (("pk_x4=0", (1, 2)), ("pk_ws=0", (1,)), ("pk_vec=0", (1, 2, 3, 4)), ("xcd_remap=0", (1, 2, 3))):
        for f in fams:
            assert (got["explicit/" + key][f] != a[f]).any(), "%s changes no %s plan of the census" % (key, FAMILIES[f])
    for v in range(7):
        assert set(got["explicit/x3_variant=%d" % v][3, :, -16][got["explicit/x3_variant=%d" % v][3, :, 0] == 0]) == {v}


def test_plans_match_the_recorded_census(got):
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(got)
    for name in sorted(got):
        g = gold[name]
        assert g.shape == got[name].shape, name
        if not np.array_equal(g, got[name]):
            if g.ndim != 3:
                raise AssertionError("%s differs from the recorded census" % name)
            f, i = np.argwhere((g != got[name]).any(axis=2))[0]
            a = explicit_rows()[i][0]
            raise AssertionError("%s, family %s, row %d (%s):\n recorded %s\n now      %s" % (
                name, FAMILIES[f], i, {n: getattr(a, n) for n, _ in a._fields_ if isinstance(getattr(a, n), (int, float))},
                g[f, i].tolist(), got[name][f, i].tolist()))


if __name__ == "__main__":
    if "--record" in sys.argv:
        np.savez_compressed(GOLDEN, **census())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
