"""Flat-buffer AdamW launches (host-scalar and device-record forms).

Part of `vcvits_amd.ops` (the package re-exports every name: `from vcvits_amd import ops; ops.conv1d(...)`).  Everything here
runs on the GPU through libvcvits_hip.so; there is no CPU fallback."""

from .._lib import (check, lib, ptr, stream)


# ---------------------------------------------------------------------------------------------
# AdamW on flat buffers
# ---------------------------------------------------------------------------------------------
def adamw_step(p, g, m, v, lr, betas, eps, weight_decay, step):
    check(lib().vcv_adamw(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps,
                          weight_decay, step, stream()), "vcv_adamw")


def adamw_step_dev(p, g, m, v, betas, eps, weight_decay, hyper, step_base):
    """The same step with lr and the step delta read from the device record `hyper` (int32[2]: fp32 bits of lr, delta):
    the form an optimizer step recorded into a HIP graph takes (light/graphed.py refreshes the record before each replay)."""
    check(lib().vcv_adamw_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), betas[0], betas[1], eps, weight_decay,
                              ptr(hyper), int(step_base), stream()), "vcv_adamw_dev")


# ---------------------------------------------------------------------------------------------
# gradient norms of segments of a flat buffer, and AdamW with the clip coefficient read from device memory
# ---------------------------------------------------------------------------------------------
GRAD_SQNORM_MAX_SEGMENTS = 8        # (csrc/elementwise.hip: GN_MAXS)
GRAD_SQNORM_WS_PER_SEGMENT = 1024   # fp64 partials per segment (GN_MAXB)


def grad_sqnorm_record_bytes(n_segments):
    """Bytes of the result record of `grad_sqnorm`: double sq[S]; float norm[S]; float total_norm; float coef."""
    return 12 * int(n_segments) + 8


def grad_sqnorm(buf, segs, n_segments, ws, rec, max_norm=0.0):
    """Squared L2 norms of `n_segments` segments of the flat fp32 buffer `buf` into the record `rec`, through the workspace
    `ws` (float64, n_segments * 1024): two launches, no atomics, no sync, capturable.  `segs` is a DEVICE int64 tensor of
    (lo, hi) element offsets whose rows the caller has checked against `buf.numel()` (the launcher does not read them);
    max_norm <= 0 / inf: no clipping, the record's coefficient is exactly 1.0."""
    S = int(n_segments)
    if not (buf.is_cuda and segs.is_cuda and ws.is_cuda and rec.is_cuda):
        raise RuntimeError("vcvits_amd: grad_sqnorm needs GPU tensors; the HIP path has no CPU fallback")
    import torch
    if buf.dtype != torch.float32 or segs.dtype != torch.int64 or ws.dtype != torch.float64:
        raise TypeError("grad_sqnorm: buf must be float32, segs int64, ws float64")
    if not 0 < S <= GRAD_SQNORM_MAX_SEGMENTS or segs.numel() < 2 * S or ws.numel() < S * GRAD_SQNORM_WS_PER_SEGMENT \
            or rec.numel() * rec.element_size() < grad_sqnorm_record_bytes(S):
        raise ValueError("grad_sqnorm: %d segments need a table of %d int64, a workspace of %d float64 and a record of %d bytes"
                         % (S, 2 * S, S * GRAD_SQNORM_WS_PER_SEGMENT, grad_sqnorm_record_bytes(S)))
    check(lib().vcv_grad_sqnorm(ptr(buf), ptr(segs), S, ptr(ws), ptr(rec), float(max_norm), stream()), "vcv_grad_sqnorm")


def adamw_step_clip(p, g, m, v, lr, betas, eps, weight_decay, step, coef):
    """`adamw_step` on g * coef[0] (`coef`: a device fp32 scalar, e.g. the record of `grad_sqnorm`); g is not written."""
    check(lib().vcv_adamw_clip(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay, step,
                               ptr(coef), stream()), "vcv_adamw_clip")


def adamw_step_dev_clip(p, g, m, v, betas, eps, weight_decay, hyper, step_base, coef):
    """`adamw_step_dev` on g * coef[0]: the form a clipped optimizer step recorded into a HIP graph takes."""
    check(lib().vcv_adamw_dev_clip(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), betas[0], betas[1], eps, weight_decay,
                                   ptr(hyper), int(step_base), ptr(coef), stream()), "vcv_adamw_dev_clip")


def set_hyper(hyper, lr, delta):
    import struct
    check(lib().vcv_set_words(ptr(hyper), 2, struct.unpack("<i", struct.pack("<f", float(lr)))[0], int(delta), 0, 0, stream()),
          "vcv_set_words")
