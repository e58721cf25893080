"""The fused relative-position attention kernels (csrc/attention.hip: seven kernels behind vcv_rel_attn_fwd / _bwd2 / _bwd) at
the edges of their launchers, against a float64 CPU reference of the same operation (tests/attention_f64.py).

The kernels are called THROUGH THE C ABI (vcvits_amd._lib.lib().vcv_rel_attn_*), so the routing of ops.rel_attention cannot
send a case elsewhere; test_routing_* then check that ops.rel_attention reaches the same kernels (same bits) and that the
shapes the fused kernels refuse run on the unfused path of csrc/vits_blocks.hip within the same bounds.

Reference: attention_f64.rel_attention on float64 copies of the float32 inputs, float64 autograd of the same expression for
the five gradients.  Dropout: the keep mask is attention_f64.keep_mask(seed, ...), the integer restatement of the kernels'
counter-based generator, an INPUT of the reference -- and compared exactly with the zeros of the kernel's Pd.

Distances are max|a - b| / max|b|.  Bounds: for every (case, tensor) d32 is the distance of the FLOAT32 CPU run of
attention_f64 from its float64 run (the reference against itself, never the kernel); the fp32-mode bound is
max(FACTOR * d32, 2e-6), capped by the project's 1e-4 (2e-4 for the two relative tables; tests/test_attention_full_gpu.py).
FACTOR = 16 covers the kernels' __expf / exp2 intrinsics and their other summation order; the floor is there because d32 is 0
at T = 1.  bf16 mode: see test_bf16_mode.

Every GPU case writes its distances to profiles/attention_parity.txt.

The CPU tests at the top (not marked gpu) pin the reference itself: to oracle.vits_oracle.rel_attention and
tests/golden/attention.npz, and keep_mask to its expected share; and the case table to the launchers' rules."""
import collections
import contextlib
import functools
import math
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_f64 as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1  # VCV_EINVAL (include/vcvits_hip.h)
FACTOR, FLOOR, CAP, CAP_TABLE = 16, 2e-6, 1e-4, 2e-4
TOL_BF16_GRAD = 3e-2  # tests/test_attention_fused_gpu.py
GUARD, SENT = 1024, 12345.0

Case = collections.namedtuple("Case", "B H dk T w mask bwd")  # bwd: "bwd2" (with the forward's out) or "bwd" (null out)


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' rules, restated (attention.hip: ok_shape, vcv_rel_attn_fwd, vcv_rel_attn_bwd2)
# ---------------------------------------------------------------------------------------------------------------------
NWV, RELP, FW, RWP, PTP, CK = 8, 16, 4, 17, 33, 128
BSF = max(64 * (CK + 2), NWV * 32 * 33)
LDS_LIMIT, LDS_STATIC = 160 * 1024, 64 * 1024


def cdiv(a, b):
    return -(-a // b)


def tp_of(T):
    return ((T + 63) & ~63) + 2


def lds_bytes(TP):
    return 4 * (32 * TP + 32 * RELP + TP + RELP * 64 + BSF)


def lds_rows(dk, nkt=8):
    return 4 * (nkt * 32 + 2 * dk * (nkt * 32 + 1) + RELP * dk + FW * (32 * RWP + 32 * PTP))


def lds_bwd_rows2(dk, nkt=8):
    return 4 * (dk * (nkt * 32 + 1) + RELP * dk + FW * (3 * 32 * RWP + 32 * PTP))


def lds_bwd_cols2(dk, nkt=8):
    return 4 * (2 * dk * (nkt * 32 + 1))


def ok_shape(B, H, dk, T, w):
    return B > 0 and H > 0 and 0 < dk <= 64 and dk % 2 == 0 and T > 0 and w >= 0 and 2 * w + 1 <= RELP and \
        lds_bytes(tp_of(T)) <= LDS_LIMIT


def plan(B, H, dk, T, w, with_out=True):
    """Which kernels the two launchers pick, whether they take the dynamic-LDS attribute call (lds > 64 KiB), and the
    geometry the case list speaks of."""
    if not ok_shape(B, H, dk, T, w):
        return {"fwd": "UNSUPPORTED", "bwd": "UNSUPPORTED"}
    rows = T <= 256 and dk in (32, 64) and 2 * w + 1 <= RELP
    nkt = cdiv(T, 32)
    p = {"fwd": "ROWS" if rows else "TILE", "bwd": "ROWS2" if rows and with_out else "TILE", "tiles": nkt,
         "chunks": cdiv(T, CK), "last_chunk": T - CK * (cdiv(T, CK) - 1), "channel_tiles": cdiv(dk, 32)}
    tile_attr = lds_bytes(tp_of(T)) > LDS_STATIC
    p["fwd_attr"] = lds_rows(dk) > LDS_STATIC if rows else tile_attr
    # backward: the row kernel's attribute call (ROWS2: either of its two kernels; TILE: the column kernel's 2 * BSF floats are
    # past 64 KiB at every shape, so only the row kernel's depends on the case)
    p["bwd_attr"] = (lds_bwd_rows2(dk) > LDS_STATIC or lds_bwd_cols2(dk) > LDS_STATIC) if p["bwd"] == "ROWS2" else tile_attr
    if rows:
        p["wgs"] = cdiv(nkt, FW)
        p["idle_waves"] = p["wgs"] * FW - nkt
    else:
        p["tiles_of_wave0"] = cdiv(nkt, NWV)
    return p


# (case, what plan() must say of it)
TABLE = [
    # ---- one wave per 32 queries (T <= 256, dk 32 / 64)
    (Case(1, 1, 32, 1, 4, "ones", "bwd2"), {"fwd": "ROWS", "bwd": "ROWS2", "tiles": 1}),           # one query, one key: r = w alone
    (Case(2, 1, 32, 5, 7, "ragged", "bwd2"), {"fwd": "ROWS", "bwd": "ROWS2"}),                      # T <= w: band clipped on both sides
    (Case(2, 2, 64, 32, 0, "hole", "bwd2"), {"fwd": "ROWS", "bwd": "ROWS2", "tiles": 1}),           # w = 0, an exact tile
    (Case(2, 1, 64, 33, 4, "ragged", "bwd2"), {"fwd": "ROWS", "bwd": "ROWS2", "tiles": 2}),         # the second tile holds one row
    (Case(1, 2, 32, 128, 4, "ones", "bwd2"), {"fwd": "ROWS", "tiles": 4, "wgs": 1, "idle_waves": 0}),  # FW tiles, unmasked copy
    (Case(2, 1, 32, 129, 7, "ragged+hole", "bwd2"), {"fwd": "ROWS", "tiles": 5, "wgs": 2, "idle_waves": 3}),
    (Case(2, 2, 64, 256, 4, "ragged+hole", "bwd2"), {"fwd": "ROWS", "bwd": "ROWS2", "tiles": 8, "wgs": 2, "idle_waves": 0,
                                                     "fwd_attr": True, "bwd_attr": True}),
    (Case(3, 1, 32, 97, 4, "mixed", "bwd2"), {"fwd": "ROWS", "bwd": "ROWS2", "tiles": 4}),          # ones | ragged | all zero
    # ---- workgroup per 32 queries: forward and backward
    (Case(2, 1, 32, 257, 4, "ragged+hole", "bwd2"), {"fwd": "TILE", "bwd": "TILE", "tiles": 9, "tiles_of_wave0": 2}),
    (Case(2, 1, 64, 896, 4, "ragged", "bwd2"), {"fwd": "TILE", "bwd": "TILE", "tiles": 28, "fwd_attr": True}),
    (Case(1, 2, 64, 513, 1, "ones", "bwd2"), {"fwd": "TILE", "tiles": 17, "chunks": 5, "last_chunk": 1}),
    (Case(2, 1, 16, 130, 4, "ragged", "bwd2"), {"fwd": "TILE", "bwd": "TILE", "chunks": 2, "last_chunk": 2}),
    (Case(1, 1, 32, 384, 4, "ones", "bwd2"), {"fwd": "TILE", "chunks": 3, "last_chunk": 128}),
    (Case(2, 2, 2, 37, 4, "hole", "bwd2"), {"fwd": "TILE", "bwd": "TILE", "fwd_attr": False}),
    (Case(2, 1, 8, 37, 4, "ragged", "bwd2"), {"fwd": "TILE", "bwd": "TILE"}),
    (Case(2, 1, 48, 70, 3, "ragged+hole", "bwd2"), {"fwd": "TILE", "bwd": "TILE", "channel_tiles": 2}),
    (Case(1, 1, 62, 40, 7, "ones", "bwd2"), {"fwd": "TILE", "bwd": "TILE", "channel_tiles": 2}),
    # the workgroup-per-tile BACKWARD at shapes whose forward is ROWS: vcv_rel_attn_bwd (null `out`)
    (Case(2, 2, 32, 31, 4, "ragged", "bwd"), {"fwd": "ROWS", "bwd": "TILE", "bwd_attr": False}),
    (Case(2, 1, 64, 225, 4, "ragged", "bwd"), {"fwd": "ROWS", "bwd": "TILE", "bwd_attr": True}),
]
CASES = [c for c, _ in TABLE]
# p = 0 and 0.1 everywhere; p = 0.5 on two cases of each family
P_HALF = {Case(2, 1, 64, 33, 4, "ragged", "bwd2"), Case(3, 1, 32, 97, 4, "mixed", "bwd2"),
          Case(2, 1, 16, 130, 4, "ragged", "bwd2"), Case(2, 1, 48, 70, 3, "ragged+hole", "bwd2")}
CASE_P = [(c, p) for c in CASES for p in ((0.0, 0.1, 0.5) if c in P_HALF else (0.0, 0.1))]
# bf16 mode: two ROWS and two TILE cases
BF16_CASES = [Case(2, 1, 64, 33, 4, "ragged", "bwd2"), Case(2, 1, 32, 129, 7, "ragged+hole", "bwd2"),
              Case(2, 1, 32, 257, 4, "ragged+hole", "bwd2"), Case(2, 1, 48, 70, 3, "ragged+hole", "bwd2")]
# the dropout seed of this case lies past 2^63 (uint64 wrap in seed + idx * constant)
BIG_SEED_CASE = Case(2, 1, 32, 129, 7, "ragged+hole", "bwd2")


def cid(c):
    return "B%d-H%d-dk%d-T%d-w%d-%s-%s" % tuple(c)


def plan_of(c):
    return plan(c.B, c.H, c.dk, c.T, c.w, with_out=c.bwd == "bwd2")


def make_mask(c):
    B, T = c.B, c.T
    m = torch.ones(B, T)
    if c.mask == "mixed":  # element 0 all ones, element 1 ragged, element 2 all zero
        m[1, T - T // 5:] = 0.0
        m[2, :] = 0.0
        return m
    if "ragged" in c.mask:
        m[B - 1, T - T // 5:] = 0.0
    if "hole" in c.mask:
        m[0, T // 3] = 0.0
    return m


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the reference itself, and the case table
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_matches_oracle_and_golden():
    """attention_f64.rel_attention between the module's 1x1 convolutions against oracle.vits_oracle.rel_attention and the
    vectors of tests/golden/attention.npz (d_k = 8, window 4, one ragged row), at tests/test_oracle_vs_golden.py's 2e-5: output
    and probabilities, and through conv_o / conv_q,k,v the gradients of x and of the two relative tables.  With a keep mask:
    against the oracle's `drop` hook."""
    from golden_util import fill_state_dict, keys_shapes_of, load
    from oracle import vits_oracle as O
    from vcvits_amd.model.transformer.relative_attention_transformer import MultiHeadAttention
    TOL = 2e-5
    g = load("attention.npz")
    sd = fill_state_dict(keys_shapes_of(MultiHeadAttention(16, 16, 2, p_dropout=0.0, window_size=4)), int(g["seed"]))
    x = torch.from_numpy(np.asarray(g["x"]))
    T = x.shape[-1]
    xm = O.sequence_mask(torch.from_numpy(np.asarray(g["lengths"])), T).float()  # [B, T]
    am = xm.unsqueeze(1).unsqueeze(2) * xm.unsqueeze(1).unsqueeze(-1)
    conv = lambda t, n: F.conv1d(t, sd["conv_%s.weight" % n].to(t.dtype), sd["conv_%s.bias" % n].to(t.dtype))
    for dtype, tol in ((torch.float64, TOL), (torch.float32, TOL)):
        xd = x.to(dtype)
        q, k, v = conv(xd, "q"), conv(xd, "k"), conv(xd, "v")
        r = torch.from_numpy(np.asarray(g["r"])).to(dtype)
        dO = F.conv_transpose1d(r, sd["conv_o.weight"].to(dtype))  # gradient of conv_o's input
        res = A.rel_attention(q, k, v, sd["emb_rel_k"], sd["emb_rel_v"], xm, dO, dtype=dtype)
        y = conv(res.out, "o")
        yo, po = O.rel_attention({"a." + n: t for n, t in sd.items()}, "a", x, am, 2, 4)
        assert A.dist(y, yo) <= tol and A.dist(res.P.view(po.shape), po) <= tol
        assert A.dist(y, torch.from_numpy(g["y"])) <= tol and A.dist(res.P.view(po.shape), torch.from_numpy(g["attn"])) <= tol
        dx = sum(F.conv_transpose1d(gr, sd["conv_%s.weight" % n].to(dtype)) for gr, n in ((res.dq, "q"), (res.dk, "k"), (res.dv, "v")))
        assert A.dist(dx, torch.from_numpy(g["dx"])) <= tol
        assert A.dist(res.dembk, torch.from_numpy(g["dp_emb_rel_k"])) <= tol
        assert A.dist(res.dembv, torch.from_numpy(g["dp_emb_rel_v"])) <= tol
    # dropout: the oracle applies its `drop` hook where the reference module applies self.drop
    B, H = x.shape[0], 2
    keep = A.keep_mask(5, B * H * T * T, 0.3).reshape(B * H, T, T)
    kt = torch.from_numpy(keep).view(B, H, T, T).float()
    yo, po = O.rel_attention({"a." + n: t for n, t in sd.items()}, "a", x, am, 2, 4, drop=lambda p: p * kt * A.inv_keep(0.3))
    q, k, v = conv(x.double(), "q"), conv(x.double(), "k"), conv(x.double(), "v")
    res = A.rel_attention(q, k, v, sd["emb_rel_k"], sd["emb_rel_v"], xm, keep=keep, p=0.3)
    assert A.dist(conv(res.out, "o"), yo) <= TOL and A.dist(res.Pd.view(po.shape), po) <= TOL
    mb = xm.bool().repeat_interleave(H, 0)             # [B*H, T]
    ex = mb.unsqueeze(2) & ~mb.unsqueeze(1)            # masked keys of unmasked queries: P is exactly 0
    assert bool((res.P[ex] == 0).all()) and bool((((res.Pd != 0) == torch.from_numpy(keep)) | ex).all())


def _splitmix_keep(seed, idx, p):
    """One element of the stream in Python integers (the C text of drop_scale, mod 2^64 spelled out)."""
    M = (1 << 64) - 1
    z = (seed + idx * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return np.float32(z >> 40) * np.float32(1.0 / 16777216.0) >= np.float32(p)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_share(p):
    """keep_mask keeps a share within 3 sigma of 1 - p over 2^20 elements; its vectorised uint64 arithmetic agrees with the
    scalar form, also for a seed past 2^63."""
    n = 1 << 20
    share = float(A.keep_mask(77, n, p).mean())
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(share - (1 - p)) <= 3 * sigma, (share, sigma)
    for seed in (0, 77, (1 << 63) + 12345, (1 << 64) - 1):
        got = A.keep_mask(seed, 4096, p)
        assert all(bool(got[i]) == bool(_splitmix_keep(seed, i, p)) for i in range(0, 4096, 7))
    assert not A.keep_mask(77, 1 << 16, 0.5).all() and A.keep_mask(77, 1 << 16, 0.0).all()


def test_case_table_reaches_every_branch():
    """The table above against the launchers' rules as plan() restates them, and the branches the file claims to cover."""
    seen = collections.Counter()
    for c, want in TABLE:
        got = plan_of(c)
        assert {k: got.get(k) for k in want} == want, (c, want, got)
        assert c.B * c.H <= 4
        seen.update(["fwd " + got["fwd"], "bwd " + got["bwd"], "fwd_attr %s %s" % (got["fwd"], got["fwd_attr"]),
                     "bwd_attr %s %s" % (got["bwd"], got["bwd_attr"])])
        m = make_mask(c)
        for b in range(c.B):
            seen.update(["%s allone" % got["fwd"]] * bool(m[b].all()) + ["%s masked" % got["fwd"]] * (not bool(m[b].all())))
            seen.update(["all-masked element"] * (not bool(m[b].any())))
        if got["fwd"] == "ROWS":
            seen.update(["idle waves"] * (got["idle_waves"] > 0) + ["two workgroups"] * (got["wgs"] > 1))
        else:
            seen.update(["prefetch"] * (got["tiles_of_wave0"] > 1) + ["partial chunk"] * (got["last_chunk"] < CK) +
                        ["exact chunks"] * (got["last_chunk"] == CK and got["chunks"] > 1) + ["dk<32"] * (c.dk < 32) +
                        ["half-empty channel tile"] * (c.dk % 32 != 0 and c.dk > 32))
        seen.update(["T<=w"] * (c.T <= c.w) + ["w=0"] * (c.w == 0) + ["w=7"] * (c.w == 7))
    for branch in ("fwd ROWS", "fwd TILE", "bwd ROWS2", "bwd TILE", "fwd_attr ROWS True", "fwd_attr TILE True", "fwd_attr TILE False",
                   "bwd_attr ROWS2 True", "bwd_attr TILE True", "bwd_attr TILE False", "ROWS allone", "ROWS masked", "TILE allone",
                   "TILE masked", "all-masked element", "idle waves", "two workgroups", "prefetch", "partial chunk", "exact chunks",
                   "dk<32", "half-empty channel tile", "T<=w", "w=0", "w=7"):
        assert seen[branch] > 0, branch
    # the launchers' limits: the longest T, the widest window, the channel counts refused
    assert plan(1, 1, 64, 896, 4)["fwd"] == "TILE" and plan(1, 1, 64, 897, 4)["fwd"] == "UNSUPPORTED"
    assert plan(1, 1, 32, 256, 7)["fwd"] == "ROWS" and plan(1, 1, 32, 257, 7)["fwd"] == "TILE"
    for dk, w in ((66, 4), (7, 4), (32, 8), (0, 4)):
        assert plan(1, 1, dk, 64, w)["fwd"] == "UNSUPPORTED"
    assert plan(1, 1, 32, 64, 4, with_out=False)["bwd"] == "TILE"
    assert all(c in CASES for c in list(P_HALF) + BF16_CASES + [BIG_SEED_CASE])
    assert sum(plan_of(c)["fwd"] == "ROWS" for c in P_HALF) == 2 and sum(plan_of(c)["fwd"] == "ROWS" for c in BF16_CASES) == 2


# ---------------------------------------------------------------------------------------------------------------------
# inputs and float64 references: made once per case and shared by every test
# ---------------------------------------------------------------------------------------------------------------------
def seed_of(c):
    s = zlib.crc32(repr(tuple(c)).encode())
    return s + (1 << 63) + (1 << 40) if c == BIG_SEED_CASE else s


@functools.lru_cache(maxsize=None)
def inputs(c, rounded=False):
    """q, k, v, embk, embv, mask, dO (float32, CPU): standard normal, the tables scaled by dk^-0.5.  rounded: q, k, v and dO
    are bf16 numbers (the tables only meet fp32 arithmetic in the kernels)."""
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    t = lambda *sh: torch.from_numpy(rng.standard_normal(sh).astype(np.float32))
    C = c.H * c.dk
    q, k, v, dO = t(c.B, C, c.T), t(c.B, C, c.T), t(c.B, C, c.T), t(c.B, C, c.T)
    ek, ev = t(1, 2 * c.w + 1, c.dk) * c.dk ** -0.5, t(1, 2 * c.w + 1, c.dk) * c.dk ** -0.5
    if rounded:
        q, k, v, dO = (x.bfloat16().float() for x in (q, k, v, dO))
    return q, k, v, ek, ev, make_mask(c), dO


@functools.lru_cache(maxsize=None)
def keep_of(c, p, seed=None):
    if p == 0:
        return None
    G, T = c.B * c.H, c.T
    return torch.from_numpy(A.keep_mask(seed_of(c) if seed is None else seed, G * T * T, p).reshape(G, T, T))


@functools.lru_cache(maxsize=None)
def reference(c, p, rounded=False, seed=None):
    """(float64 Result, {tensor: d32}): d32 = distance of the float32 run of the same text from the float64 run."""
    q, k, v, ek, ev, mask, dO = inputs(c, rounded)
    keep = keep_of(c, p, seed)
    r64 = A.rel_attention(q, k, v, ek, ev, mask, dO, torch.float64, keep, p)
    r32 = A.rel_attention(q, k, v, ek, ev, mask, dO, torch.float32, keep, p)
    return r64, {n: A.dist(a, b) for n, a, b in zip(A.NAMES, r32, r64)}


def bound(name, d32):
    return min(max(FACTOR * d32, FLOOR), CAP_TABLE if name.startswith("demb") else CAP)


@functools.lru_cache(maxsize=2)
def on_gpu(c, rounded, gpu):
    return tuple(t.to(gpu) for t in inputs(c, rounded))


# ---------------------------------------------------------------------------------------------------------------------
# the entry points, called directly; every output lies inside a larger buffer with sentinels on both sides
# ---------------------------------------------------------------------------------------------------------------------
class Guarded:
    """n floats pre-filled with NaN (an element left unwritten stays NaN) between two runs of GUARD sentinel floats."""

    def __init__(self, shape, device):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device=device)
        self.buf[:GUARD] = SENT
        self.buf[GUARD + n:] = SENT
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        n = self.t.numel()
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + n:] == SENT).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def abi_fwd(c, ins, p, seed, bf=0, want_p=True, want_pd=True):
    """-> status, out, P, Pd (Guarded; P / Pd None when not asked for)"""
    from vcvits_amd._lib import lib, ptr, stream
    q, k, v, ek, ev, mask, _ = ins
    G, T, dev = c.B * c.H, c.T, k.device
    out = Guarded((c.B, c.H * c.dk, T), dev)
    P = Guarded((G, T, T), dev) if want_p else None
    Pd = Guarded((G, T, T), dev) if want_pd else None
    st = lib().vcv_rel_attn_fwd(ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(mask), ptr(out.t), ptr(P.t) if P else None,
                                ptr(Pd.t) if Pd else None, c.B, c.H, c.dk, T, c.w, c.dk ** -0.5, p, seed, bf, stream())
    return st, out, P, Pd


def workspace_floats(c):
    """The documented size (include/vcvits_hip.h): dS and the per-(head, query tile) partial tables of the two table gradients."""
    return c.B * c.H * c.T * c.T + c.B * c.H * cdiv(c.T, 32) * 2 * (2 * c.w + 1) * c.dk


def abi_bwd(c, ins, P, out, p, seed, bf=0):
    """out None: vcv_rel_attn_bwd.  -> status, {dq, dk, dv, dembk, dembv: Guarded}, workspace (Guarded)"""
    from vcvits_amd._lib import lib, ptr, stream
    q, k, v, ek, ev, mask, dO = ins
    dev = k.device
    g = {n: Guarded(tuple(t.shape), dev) for n, t in (("dq", k), ("dk", k), ("dv", v), ("dembk", ek), ("dembv", ev))}
    ws = Guarded((workspace_floats(c),), dev)
    common = (ptr(ws.t), ptr(g["dq"].t), ptr(g["dk"].t), ptr(g["dv"].t), ptr(g["dembk"].t), ptr(g["dembv"].t), c.B, c.H, c.dk, c.T,
              c.w, c.dk ** -0.5, p, seed, bf, stream())
    head = (ptr(q), ptr(k), ptr(v), ptr(ek), ptr(ev), ptr(mask), ptr(P))
    if out is None:
        st = lib().vcv_rel_attn_bwd(*head, ptr(dO), *common)
    else:
        st = lib().vcv_rel_attn_bwd2(*head, ptr(out), ptr(dO), *common)
    return st, g, ws


@contextlib.contextmanager
def fp32_mode():
    from vcvits_amd import ops
    old = ops.compute_dtype()
    ops.set_compute_dtype("f32")
    try:
        yield
    finally:
        ops.set_compute_dtype(old)


_parity = {}


def record(section, line):
    """Keep the measured distances in profiles/attention_parity.txt (rewritten with every line measured so far)."""
    print(line)
    _parity.setdefault(section, [])
    if line not in _parity[section]:
        _parity[section].append(line)
    with open(os.path.join(ROOT, "profiles", "attention_parity.txt"), "w") as f:
        f.write("# tests/test_attention_abi_gpu.py: max-norm distance of the vcv_rel_attn_* entry points from the float64 CPU reference\n"
                "# (tests/attention_f64.py), relative to max|reference|, as tensor=kernel/d32/bound: d32 is the distance of the float32\n"
                "# CPU run of the reference from its float64 run.  Cases are B-H-dk-T-window-mask-backward entry point.\n")
        for name in _parity:
            f.write("\n[%s]\n" % name)
            f.write("\n".join(_parity[name]) + "\n")


def check(section, tag, got, ref, d32, names, bounds=None, zero_scale=None):
    """Write the figures down first, then assert.  zero_scale: the scale a tensor is measured against where its reference is
    identically zero (see test_backward_fp32)."""
    errs = {n: A.dist(got[n], getattr(ref, n)) for n in names}
    for n in names:
        if zero_scale is not None and not bool(getattr(ref, n).any()):
            errs[n] = got[n].detach().cpu().double().abs().max().item() / zero_scale
    bounds = bounds or {n: bound(n, d32[n]) for n in names}
    record(section, "%-52s %s" % (tag, " ".join("%s=%.1e/%.1e/%.1e" % (n, errs[n], d32[n], bounds[n]) for n in names)))
    for n in names:
        assert errs[n] <= bounds[n], "%s %s: %s off by %.3e (d32 %.3e, bound %.3e)" % (section, tag, n, errs[n], d32[n], bounds[n])
    return errs


def excluded(c):
    """[G, T, T] bool: masked keys of unmasked query rows, the only elements where P is exactly 0 (on both sides), so that a
    zero of Pd says nothing about the dropout mask there."""
    m = make_mask(c).bool()
    ex = m.unsqueeze(2) & ~m.unsqueeze(1)  # [B, T(i), T(j)]
    return ex.repeat_interleave(c.H, 0)


def check_dropout_mask(c, p, P, Pd, keep, bnd):
    P, Pd = P.cpu(), Pd.cpu()
    ex = excluded(c)
    assert bool((P[ex] == 0).all()) and bool((Pd[ex] == 0).all()), "a masked key of an unmasked query has a probability"
    assert bool((P[~ex] > 0).all()), "a probability outside the masked keys is zero"
    if p > 0:
        wrong = ((Pd != 0) != keep) & ~ex
        assert not bool(wrong.any()), "%d elements dropped / kept against keep_mask, first at %s" % (
            int(wrong.sum()), tuple(int(x) for x in wrong.nonzero()[0]))
        want = P.double() * keep.double() * A.inv_keep(p)  # the kernel's own P through the given mask
        assert A.dist(Pd, want) <= bnd, ("Pd != P * keep / (1 - p)", A.dist(Pd, want), bnd)
    else:
        assert torch.equal(P, Pd)


def tag_of(c, p):
    pl = plan_of(c)
    return "%s %s/%s p=%g" % (cid(c), pl["fwd"], pl["bwd"], p)


case_p_ids = lambda cp: "%s-p%g" % (cid(cp[0]), cp[1])


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward, fp32 mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cp", CASE_P, ids=case_p_ids)
def test_forward_fp32(gpu, cp):
    c, p = cp
    ins, seed = on_gpu(c, False, gpu), seed_of(c)
    ref, d32 = reference(c, p)
    runs = {}
    for want_p, want_pd in ((True, True), (True, False), (False, True), (False, False)):
        st, out, P, Pd = abi_fwd(c, ins, p, seed, 0, want_p, want_pd)
        assert st == 0, st
        for name, gd in (("out", out), ("P", P), ("Pd", Pd)):
            if gd is not None:
                assert gd.intact(), "%s: a write outside the buffer" % name
                assert not bool(torch.isnan(gd.t).any()), "%s has elements the kernel did not write" % name
        runs[want_p, want_pd] = (out.t, P.t if P else None, Pd.t if Pd else None)
    out, P, Pd = runs[True, True]
    for key, (o2, P2, Pd2) in runs.items():
        assert torch.equal(out, o2), "out differs with (P, Pd) = %s" % (key,)
        assert P2 is None or torch.equal(P, P2), "P differs between two runs"
        assert Pd2 is None or torch.equal(Pd, Pd2), "Pd differs between two runs"
    check("forward fp32", tag_of(c, p), {"out": out, "P": P, "Pd": Pd}, ref, d32, ("out", "P", "Pd"))
    check_dropout_mask(c, p, P, Pd, keep_of(c, p), bound("Pd", d32["Pd"]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. backward, fp32 mode
# ---------------------------------------------------------------------------------------------------------------------
GRADS = ("dq", "dk", "dv", "dembk", "dembv")


def cancel_scale(c, ref):
    """T = 1: the softmax of one score has no derivative, so dq, dk and dembk are exactly zero in the reference and max|ref| is
    no scale.  The kernels form dS = P (dPd - dot) from two equal numbers that they sum in different orders (dPd = dO . (v +
    embv) on the matrix cores and in the band product, dot = sum_d dO out), and multiply the difference by qscale and by q, k or
    embk: the result is measured against qscale * max|dot| * max(|q|, |k|, |embk|), the size of the terms that cancel."""
    q, k, _, ek, _, _, dO = inputs(c)
    dot = (dO.double() * ref.out).view(c.B, c.H, c.dk, c.T).sum(2).abs().max().item()
    return c.dk ** -0.5 * dot * max(t.abs().max().item() for t in (q, k, ek)) + 1e-300


@pytest.mark.gpu
@pytest.mark.parametrize("cp", CASE_P, ids=case_p_ids)
def test_backward_fp32(gpu, cp):
    c, p = cp
    ins, seed = on_gpu(c, False, gpu), seed_of(c)
    ref, d32 = reference(c, p)
    st, out, P, _ = abi_fwd(c, ins, p, seed, 0, True, False)
    assert st == 0, st
    runs = []
    for _ in range(2):
        st, g, ws = abi_bwd(c, ins, P.t, out.t if c.bwd == "bwd2" else None, p, seed)
        assert st == 0, st
        assert ws.intact(), "a write outside the documented workspace"
        for n in GRADS:
            assert g[n].intact(), "%s: a write outside the buffer" % n
            assert not bool(torch.isnan(g[n].t).any()), "%s has elements the kernels did not write (or read an unwritten workspace word)" % n
        runs.append({n: g[n].t for n in GRADS})
    check("backward fp32", tag_of(c, p), runs[0], ref, d32, GRADS, zero_scale=cancel_scale(c, ref))
    # repeatability: the table gradients of the wave-per-tile backward are summed in index order (rel_attn_demb_reduce_kernel);
    # the workgroup-per-tile backward adds them with atomics
    for n in ("dq", "dk", "dv") + (("dembk", "dembv") if plan_of(c)["bwd"] == "ROWS2" else ()):
        assert torch.equal(runs[0][n], runs[1][n]), "%s differs between two identical launches" % n


# ---------------------------------------------------------------------------------------------------------------------
# 3. bf16 mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("c", BF16_CASES, ids=cid)
def test_bf16_mode(gpu, c, p):
    """bf16 = 1 on q, k, v, dO that are bf16 numbers already: the first contraction (scores, dPd) is then exact up to fp32
    accumulation, the band terms are fp32 in the code, so P is within the fp32 bound.  In the second contraction only the
    probability operand is rounded, by at most 2^-9 relative per element (8 significant bits, round to nearest) after the row
    sum was formed, and v is exact: elementwise |out - ref| <= 2^-8 * (Pd_ref @ |v|) + fp32 slack (2^-8: a factor 2 over
    2^-9; slack: the fp32 bound times max|ref|).  The gradients round dS and Pd too and keep the project's 3e-2, measured
    here against float64."""
    ins, seed = on_gpu(c, True, gpu), seed_of(c)
    ref, d32 = reference(c, p, True)
    st, out, P, Pd = abi_fwd(c, ins, p, seed, 1, True, True)
    assert st == 0, st
    assert out.intact() and P.intact() and Pd.intact()
    v = inputs(c, True)[2].double()
    B, H, dk, T = c.B, c.H, c.dk, c.T
    reach = (ref.Pd.view(B, H, T, T) @ v.view(B, H, dk, T).transpose(2, 3).abs()).transpose(2, 3).reshape(B, H * dk, T)
    slack = bound("out", d32["out"]) * ref.out.abs().max().item()
    err = (out.t.cpu().double() - ref.out).abs()
    worst = (err / (2.0 ** -8 * reach + slack)).max().item()
    tag = "%s bf16" % tag_of(c, p)
    record("bf16 mode: out, elementwise", "%-52s max|out-ref|/(2^-8 Pd|v| + slack)=%.2f  max-norm distance=%.1e" % (tag, worst, A.dist(out.t, ref.out)))
    assert worst <= 1.0, worst
    check("bf16 mode: probabilities", tag, {"P": P.t, "Pd": Pd.t}, ref, d32, ("P", "Pd"))
    check_dropout_mask(c, p, P.t, Pd.t, keep_of(c, p), bound("Pd", d32["Pd"]))
    st, g, ws = abi_bwd(c, ins, P.t, out.t, p, seed, 1)
    assert st == 0, st
    assert ws.intact() and all(g[n].intact() and not bool(torch.isnan(g[n].t).any()) for n in GRADS)
    check("bf16 mode: gradients", tag, {n: g[n].t for n in GRADS}, ref, d32, GRADS, {n: TOL_BF16_GRAD for n in GRADS})


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals: VCV_EINVAL, nothing launched, the outputs untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    from vcvits_amd._lib import lib, ptr, stream
    tried = []

    def attempt(B, H, dk, T, w, p=0.0, null_q=False, expect=EINVAL):
        """Every buffer has the size the shape asks for, so a launch that should not happen stays in bounds."""
        c = Case(B, H, dk, T, w, "ones", "bwd2")
        g0 = torch.Generator().manual_seed(9)
        C = H * dk
        q, k, v, dO = (torch.randn(B, C, T, generator=g0).to(gpu) for _ in range(4))
        ek, ev = (torch.randn(1, 2 * w + 1, dk, generator=g0).to(gpu) for _ in range(2))
        mask = torch.ones(B, T, device=gpu)
        ins = (q, k, v, ek, ev, mask, dO)
        what = "B%d-H%d-dk%d-T%d-w%d p=%g%s" % (B, H, dk, T, w, p, " null q" if null_q else "")
        if not null_q and p == 0.0:
            assert lib().vcv_rel_attn_supported(B, H, dk, T, w) == expect, "supported " + what
        qq = None if null_q else q
        st, out, P, Pd = abi_fwd(c, (qq,) + ins[1:], p, 3, 0, True, True)
        torch.cuda.synchronize()
        assert st == expect, "fwd %s returned %d" % (what, st)
        if expect == EINVAL:
            assert out.untouched() and P.untouched() and Pd.untouched(), "fwd %s wrote to an output" % what
        Pin = torch.full((B * H, T, T), 1.0 / T, device=gpu)
        oin = torch.zeros(B, C, T, device=gpu)
        st, g, ws = abi_bwd(c, (qq,) + ins[1:], Pin, oin, p, 3)
        torch.cuda.synchronize()
        assert st == expect, "bwd2 %s returned %d" % (what, st)
        if expect == EINVAL:
            assert ws.untouched() and all(g[n].untouched() for n in GRADS), "bwd2 %s wrote to an output" % what
        else:
            assert not any(bool(torch.isnan(g[n].t).any()) for n in GRADS)
        tried.append(what)

    attempt(1, 1, 64, 897, 4)   # one frame past the longest T
    attempt(1, 1, 66, 40, 4)    # more than 64 channels per head
    attempt(1, 1, 7, 40, 4)     # an odd channel count
    attempt(1, 1, 32, 40, 8)    # 2 w + 1 = 17 relative positions
    attempt(1, 1, 32, 40, 4, p=1.0)
    attempt(1, 1, 32, 40, 4, p=-0.25)
    attempt(1, 1, 32, 40, 4, null_q=True)
    # the same buffers' shape is accepted when nothing is wrong with the call (the refusals above are not a broken call)
    attempt(1, 1, 32, 40, 4, expect=0)
    attempt(1, 1, 64, 896, 4, expect=0)
    record("refusals", "%d calls refused with VCV_EINVAL, outputs untouched: %s" % (len(tried) - 2, "; ".join(tried[:-2])))


# ---------------------------------------------------------------------------------------------------------------------
# 5. routing: ops.rel_attention
# ---------------------------------------------------------------------------------------------------------------------
def _through_ops(gpu, c, p, state=77):
    """ops.rel_attention in training mode with the dropout stream at `state` -> tensors by name, the seed it drew, and the
    number of fused launches."""
    from vcvits_amd import ops
    from vcvits_amd.ops import blocks
    q, k, v, ek, ev, mask, dO = on_gpu(c, False, gpu)
    ts = [t.clone().requires_grad_(True) for t in (q, k, v, ek, ev)]
    ops.set_seed_state(state)
    old, blocks.DROPOUT_TRACE[0] = blocks.DROPOUT_TRACE[0], []
    try:
        before = ops.LAUNCH_COUNTS["attn_fused"]
        out, attn = ops.rel_attention(*ts, mask, c.H, c.w, p, training=True, want_attn=True)
        out.backward(dO)
        fused = ops.LAUNCH_COUNTS["attn_fused"] - before
        trace = blocks.DROPOUT_TRACE[0]
    finally:
        blocks.DROPOUT_TRACE[0] = old
    seed = 0
    if p > 0:
        assert len(trace) == 1 and trace[0][0] == "attn" and trace[0][3] == (c.B * c.H, c.T, c.T), trace
        seed = trace[0][2]
    got = {"out": out.detach(), "Pd": attn.detach().reshape(c.B * c.H, c.T, c.T)}
    got.update({n: t.grad for n, t in zip(GRADS, ts)})
    return got, seed, fused


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("c", [Case(1, 1, 32, 897, 4, "ragged+hole", "bwd2"), Case(2, 2, 7, 20, 2, "ragged+hole", "bwd2")], ids=cid)
def test_routing_unsupported_shapes_run_unfused(gpu, c, p):
    """One frame past the fused kernels' longest T, and an odd channel count: ops.rel_attention launches no fused kernel, and
    the unfused kernels of csrc/vits_blocks.hip meet float64 and keep_mask at the same bounds."""
    assert plan_of(c)["fwd"] == "UNSUPPORTED"
    with fp32_mode():
        got, seed, fused = _through_ops(gpu, c, p)
    assert fused == 0, "a fused launch at a shape the fused kernels refuse"
    ref, d32 = reference(c, p, False, seed if p > 0 else None)
    names = ("out", "Pd") + GRADS
    assert all(bool(torch.isfinite(got[n]).all()) for n in names)
    check("routing: unfused path", "%s p=%g" % (cid(c), p), got, ref, d32, names)
    if p > 0:
        keep = keep_of(c, p, seed)
        wrong = ((got["Pd"].cpu() != 0) != keep) & ~excluded(c)
        assert not bool(wrong.any()), "%d elements dropped / kept against keep_mask" % int(wrong.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("c", [Case(2, 1, 64, 33, 4, "ragged", "bwd2"), Case(2, 2, 64, 256, 4, "ragged+hole", "bwd2"),
                               Case(2, 1, 16, 130, 4, "ragged", "bwd2")], ids=cid)
def test_routing_same_bits_as_direct_calls(gpu, c):
    """ops.rel_attention at table rows: one fused launch, and the bits of the direct calls with the seed it drew."""
    p = 0.1
    ins = on_gpu(c, False, gpu)
    with fp32_mode():
        got, seed, fused = _through_ops(gpu, c, p)
    assert fused == 1
    st, out, P, Pd = abi_fwd(c, ins, p, seed, 0, True, True)
    assert st == 0
    st, g, _ = abi_bwd(c, ins, P.t, out.t, p, seed)
    assert st == 0
    assert torch.equal(got["out"], out.t) and torch.equal(got["Pd"], Pd.t), "ops.rel_attention: not vcv_rel_attn_fwd's bits"
    for n in ("dq", "dk", "dv") + (("dembk", "dembv") if plan_of(c)["bwd"] == "ROWS2" else ()):
        assert torch.equal(got[n], g[n].t), "ops.rel_attention: %s is not vcv_rel_attn_bwd2's bits" % n
    record("routing: fused path", "%s: ops.rel_attention == direct calls, bit for bit (seed %d)" % (tag_of(c, p), seed))
