"""The output of the relative-position self-attention for a GIVEN LIST OF QUERY ROWS (test oracle only).

tests/attention_f64.py forms [B, H, T, T] scores; at T = 20,000 that does not fit.  This file restates points 1, 2 and 4 of
that file (no dropout, no gradients) for R query rows against all T keys, so the largest tensor is [B, H, R, T].  Plain
torch-CPU code with explicit band indexing, in the dtype it is asked for; it shares no code with vcvits_amd and none with
attention_f64 (tests/test_attention_stream_cpu.py pins the two to each other: equal in float64).

 1. scores[i][j] = (q_i / sqrt(dk)) . k_j + (q_i / sqrt(dk)) . embk[j - i + w] for |j - i| <= w.
 2. scores.masked_fill(mask_i * mask_j == 0, -1e4), softmax over all T keys.
 4. out_i = sum_j P[i][j] v_j + sum_{|j - i| <= w} P[i][j] embv[j - i + w].
"""
import math

import torch


def rel_attention_rows(q, k, v, embk, embv, mask, rows, dtype=torch.float64):
    """q, k, v [B, H*dk, T]; embk, embv [1, 2w+1, dk]; mask [B, T]; rows: query indices (list / 1-d tensor, any order)
    -> out[:, :, rows] as [B, H*dk, R] in `dtype`."""
    B, C, T = q.shape
    nr, dk = embk.shape[-2], embk.shape[-1]
    w, H = (nr - 1) // 2, C // dk
    assert C == H * dk and nr == 2 * w + 1 and tuple(mask.shape) == (B, T)
    rows = torch.as_tensor(rows, dtype=torch.long).reshape(-1)
    R = rows.numel()
    assert R > 0 and int(rows.min()) >= 0 and int(rows.max()) < T
    q, k, v, ek, ev, m = (t.detach().to("cpu", dtype) for t in (q, k, v, embk, embv, mask))
    qs = q.view(B, H, dk, T)[:, :, :, rows].transpose(2, 3) / math.sqrt(dk)     # [B, H, R, dk]
    kh = k.view(B, H, dk, T).transpose(2, 3)                                      # [B, H, T, dk]
    vh = v.view(B, H, dk, T).transpose(2, 3)
    off = torch.arange(T).unsqueeze(0) - rows.unsqueeze(1) + w                    # [R, T]: j - i + w
    band = (off >= 0) & (off <= 2 * w)
    offc = off.clamp(0, 2 * w)
    scores = qs @ kh.transpose(2, 3)                                              # [B, H, R, T]
    rel = qs @ ek[0].t()                                                          # [B, H, R, 2w+1]
    scores = scores + torch.gather(rel, 3, offc.expand(B, H, R, T)) * band
    am = (m[:, rows].unsqueeze(2) * m.unsqueeze(1)).unsqueeze(1)                  # [B, 1, R, T]: mask_i * mask_j
    P = torch.softmax(scores.masked_fill(am == 0, -1e4), dim=-1)
    jr = rows.unsqueeze(1) + torch.arange(nr).unsqueeze(0) - w                    # [R, 2w+1]: the key of band entry r
    ok = (jr >= 0) & (jr < T)
    pw = torch.gather(P, 3, jr.clamp(0, T - 1).expand(B, H, R, nr)) * ok
    return (P @ vh + pw @ ev[0]).transpose(2, 3).reshape(B, C, R)
