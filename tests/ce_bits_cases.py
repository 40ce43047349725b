"""The cases and the digest behind tests/golden/ce_parent_bits.json: every output bit of the five klab_ce_* entry points
(csrc/ce.hip) at the dispatch boundaries, recorded once from the commit before the three cross-entropy files became one
(tools/record_ce_bits.py) and demanded of every tree since (tests/test_ce_parent_bits_gpu.py).

Inputs are the CPU-generated fixtures of rowops_ref.ce_case, loss_opts_ref.opts_case and distill_ref.distill_case in the guarded,
sentinel-padded buffers of the other loss tests (ld = V + 16, ldt = V + 24).  One SHA-256 per case over the raw bytes of the logits
buffer with its sentinel columns, inv, loss_row, kl_row (distillation only) and loss, in that order.

entry point   cases per shape
  plain       write_grad 0, 1, and 3 after klab_ce_count
  options     (eps, z) in {(0, 0), (0.3, 0.05)} x weights off / on x write_grad 0 / 1
  distill     every teacher dtype that fits the width x {(0, 0, no weights), (0.3, 0.05, weights)} x (alpha, T) in
              {(0, 1), (0.5, 1), (0.3, 0.5)} x write_grad 0 / 1"""
import hashlib

import torch

from tests import distill_ref as DR
from tests import loss_opts_ref as LR
from tests.rowops_ref import CE_PAD, CE_SENT, CE_V, Guarded, ce_case

F32 = torch.float32
T_PAD, T_SENT = 24, 555.0
SHAPES = [(6, V, dt) for dt in ("bf16", "f32") for V in CE_V[dt]] + [(261, 2056, "bf16"), (261, 1028, "f32")]
OPTIONS = ((0.0, 0.0), (0.3, 0.05))                  # (eps, z)
DISTILL_OPTIONS = ((0.0, 0.0, False), (0.3, 0.05, True))  # (eps, z, weights)
SETTINGS = ((0.0, 1.0), (0.5, 1.0), (0.3, 0.5))      # (alpha, T)


def shape_cases(rows, V, dt):
    """[(id, kind, parameters)] of one shape"""
    tag = f"{rows}x{V}-{dt}"
    out = [(f"plain/{tag}/wg{wg}", "plain", dict(write_grad=wg)) for wg in (0, 1, 3)]
    for eps, z in OPTIONS:
        for weighted in (False, True):
            for wg in (0, 1):
                out.append((f"opts/{tag}/eps{eps}-z{z}-w{int(weighted)}/wg{wg}", "opts", dict(eps=eps, z=z, weighted=weighted, write_grad=wg)))
    for tdt in ("bf16", "f32"):
        if V % DR.teacher_vector(tdt):
            continue
        for eps, z, weighted in DISTILL_OPTIONS:
            for alpha, T in SETTINGS:
                for wg in (0, 1):
                    out.append((f"distill/{tag}/t{tdt}/eps{eps}-z{z}-w{int(weighted)}/a{alpha}-T{T}/wg{wg}", "distill",
                                dict(tdt=tdt, eps=eps, z=z, weighted=weighted, alpha=alpha, T=T, write_grad=wg)))
    return out


def all_ids():
    return [cid for s in SHAPES for cid, _k, _p in shape_cases(*s)]


def _padded(stored, V, pad, sent):
    image = torch.full((stored.shape[0], V + pad), sent, dtype=stored.dtype)
    image[:, :V] = stored
    return Guarded(tuple(image.shape), stored.dtype, init=image)


def _digest(parts):
    h = hashlib.sha256()
    for name, g in parts:
        h.update(g.check(name).contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(ops, rows, V, dt, kind, p):
    """launch one case through `ops` and return its digest"""
    wg = p["write_grad"]
    inv, loss_row, loss = Guarded((1,), F32), Guarded((rows,), F32), Guarded((1,), F32)
    if kind == "plain":
        c = ce_case(rows, V, dt)
        buf, labels = _padded(c["stored"], V, CE_PAD, CE_SENT), c["labels"].cuda()
        if wg & 2:
            ops.ce_count(labels, inv.t)
        ops.ce_fwd(buf.t[:, :V], labels, inv.t, loss_row.t, loss.t, write_grad=wg)
        parts = [("logits", buf), ("inv", inv), ("loss_row", loss_row), ("loss", loss)]
    elif kind == "opts":
        c = LR.opts_case(rows, V, dt, p["eps"], p["z"], p["weighted"])
        buf, labels = _padded(c["stored"], V, CE_PAD, CE_SENT), c["labels"].cuda()
        w = None if c["weights"] is None else c["weights"].cuda()
        ops.ce_fwd_opts(buf.t[:, :V], labels, w, inv.t, loss_row.t, loss.t, eps=p["eps"], z=p["z"], write_grad=wg)
        parts = [("logits", buf), ("inv", inv), ("loss_row", loss_row), ("loss", loss)]
    else:
        c = DR.distill_case(rows, V, dt, p["tdt"], p["eps"], p["z"], p["weighted"], p["alpha"], p["T"])
        buf, labels = _padded(c["stored"], V, CE_PAD, CE_SENT), c["labels"].cuda()
        timage = _padded(c["teacher"], V, T_PAD, T_SENT)
        kl_row = Guarded((rows,), F32)
        w = None if c["weights"] is None else c["weights"].cuda()
        ops.ce_fwd_distill(buf.t[:, :V], timage.t[:, :V], labels, w, inv.t, loss_row.t, kl_row.t, loss.t, eps=p["eps"], z=p["z"],
                           alpha=p["alpha"], temperature=p["T"], write_grad=wg)
        parts = [("logits", buf), ("inv", inv), ("loss_row", loss_row), ("kl_row", kl_row), ("loss", loss)]
    torch.cuda.synchronize()
    return _digest(parts)


def shape_digests(ops, rows, V, dt):
    return {cid: run_case(ops, rows, V, dt, kind, p) for cid, kind, p in shape_cases(rows, V, dt)}
