"""Attention backward (csrc/attention_bwd.hip: devqa_attention_bwd, devqa_attention_bwd_f32, through lib.attention_bwd) against float64
autograd on the CPU, at the shapes the explicit backward passes run (decoder_backward of both engines, vit_backward, qformer_backward):
every path of the kernels' index space -- the second channel accumulator (dh > 64), causal sequences of several 64-row chunks, a dkdv
start chunk above 0, ko_len != q_len, strided operands and outputs, rows of no sequence, empty descriptors, large logits.

Reference (_autograd): per sequence and head, float64 scores, the mask key j <= query i + (ko_len - q_len) when causal, softmax, @ v, and
torch.autograd for d_out -- CPU tensors only, no GPU kernel in it.  Operands are rounded to the kernel's dtype before the reference sees
them; the `o` handed to the kernel is the reference output rounded to that dtype, except in case 6.  Metric: max |got - ref| / max |ref|
per output (dq, dk, dv).  Every test prints its figures before it asserts.

Bars.  fp32: 2e-5, the project's bar (test_attention_bwd_vs_autograd, test_attention_f32, test_tp_neuron_ops_gpu.py).  bf16: NOT the 6e-2
of test_attention_bwd_vs_autograd but 4 x the floor of the case, per output, computed from the reference alone when the test runs
(_floors, _bars) and never above 6e-2.  Floors: `round` = the float64 gradient rounded to bf16; `d_i` = the float64 formulas with
D_i = d_out_i . o_i taken from the bf16-rounded o (dv does not depend on D_i: 0 there); the factor 4 is for the fp32 accumulation order and
__expf.  Measured on the CPU (ranges over the cases of the group and over dq / dk / dv; `python tests/test_attention_bwd_gpu.py` prints
every line, no GPU needed):

  case 1  head dims 8, 16, 64, 65, 80, 88, 96, 128 x causal / full, lengths 1, 15, 16, 17, 63, 64, 65, 130, 200 in one call, H = 3,
          scale dh ** -0.5; and dh = 80 with scale 1.0 (OPT folds the scale into q)          test_head_dims
            round 1.2e-3 .. 3.6e-3, d_i 5.9e-4 .. 3.9e-3 (dq, dk)                             bars 4.9e-3 .. 1.6e-2
            scale 1.0: round 1.7e-3 .. 2.4e-3, d_i 5.2e-3 .. 6.0e-3                           bars 6.9e-3 .. 2.4e-2
  case 2  cross attention, 32 / 32 / 5 queries over 257 / 70 / 64 keys of another row set, dh 64 and 128, H = 2, max_len 257
                                                                                              test_cross_attention
            round 1.7e-3 .. 2.6e-3, d_i 2.7e-4 .. 4.7e-4                                      bars 7.0e-3 .. 1.1e-2
  case 3  causal with (q_len, ko_len) = (5, 70), (17, 81), (64, 130), dh 16 and 128, H = 2     test_causal_offset
            round 1.8e-3 .. 2.6e-3, d_i 1.3e-3 .. 2.2e-3                                      bars 7.3e-3 .. 1.0e-2
  case 4  fused q | k | v buffer (ld = 3 H dh), dh 80 and 128, lengths 17, 65, 130, H = 3: within the bar and the bits of the call on
          contiguous copies                                                                   test_fused_qkv_views
            round 2.0e-3 .. 2.8e-3, d_i 1.6e-3 .. 4.5e-3                                      bars 8.1e-3 .. 1.8e-2
          padded pack, dh 80, H = 2: lengths 5, 17, 64, 65, 130, 1 behind gaps of 3, 1, 7, 2, 5, 6 unowned rows (4 more at the end), NaN
          in every operand there, one descriptor with q_len = ko_len = 0 that points into a gap: gap rows of dq / dk / dv exactly 0
                                                                                              test_padded_pack
            round 1.6e-3 .. 3.0e-3, d_i 8.2e-4 .. 2.9e-3                                      bars 6.2e-3 .. 1.2e-2
          the same pack through the raw entry points into column views of one [R + 2, 3 H dh + 8] buffer full of a sentinel
                                                                                              test_output_strides
          a descriptor with q_len = 0, ko_len = 30 next to a sequence of 20, dh 65: its dk, dv exactly 0
                                                                                              test_keys_without_queries
            round 1.7e-3 .. 3.3e-3, d_i 6.2e-4 .. 1.7e-3                                      bars 6.8e-3 .. 1.3e-2
          two identical calls, same bits                                                      test_two_calls_same_bits
  case 5  large logits: dh 80, lengths 65, 130, H = 3, q and k times sqrt(32): scores of standard deviation ~32, row maxima ~100 (above
          88.7 on many rows: test_large_logit_case_is_large_cpu).  Floor `f32`: the formulas, forward included, in plain fp32 PyTorch on
          the CPU against float64; the bar is 4 x that (fp32), resp. 4 x the largest of round, d_i, f32 and <= 6e-2 (bf16)
                                                                                              test_large_logits
            fp32  causal f32 (9.2e-6, 6.6e-6, 2.8e-6)                                         bars (3.7e-5, 2.6e-5, 1.1e-5)
                  full   f32 (6.1e-6, 7.3e-6, 4.0e-6)                                         bars (2.4e-5, 2.9e-5, 1.6e-5)
            bf16  causal round (2.7e-3, 2.4e-3, 2.1e-3), d_i (6.6e-3, 6.6e-3, 0), f32 <= 5.6e-6   bars (2.6e-2, 2.7e-2, 8.4e-3)
                  full   round (2.6e-3, 2.2e-3, 2.3e-3), d_i (3.8e-3, 5.8e-3, 0), f32 <= 3.9e-6   bars (1.5e-2, 2.3e-2, 9.1e-3)
  case 6  forward then backward as production runs it: o from lib.attention on the fused operands of case 4 (the MFMA kernel in bf16,
          devqa_attention_f32 in fp32), the reference float64 end to end                      test_forward_then_backward
            fp32: 2e-5.  bf16 floor (_mfma_forward_floor): bf16 operands, fp32 scores and statistics, P rounded to bf16 for P @ v
            because it is an MFMA operand, the normaliser unrounded, o stored in bf16; the backward formulas in fp32 on that o;
            gradients stored in bf16
            dh 80   floor (3.2e-3, 3.8e-3, 2.8e-3)                                            bars (1.3e-2, 1.5e-2, 1.1e-2)
            dh 128  floor (2.2e-3, 3.7e-3, 2.5e-3)                                            bars (8.8e-3, 1.5e-2, 1.0e-2)
  case 7  dh = 129 and dh = 0: DEVQA_E_SHAPE (-2), nothing launched, pre-filled outputs untouched
                                                                                              test_bad_head_dim_is_refused_before_any_launch
  pin     descriptors with kp_len != 0: the backward ignores the visible prefix (documented, not enforced): the results are the own-key-only
          gradients.  dh 80, scale 1.0                                                        test_visible_prefix_is_ignored
            round 2.2e-3 .. 3.0e-3, d_i 4.6e-3 .. 5.8e-3                                      bars 8.7e-3 .. 2.3e-2

On the MI355X the kernels land at 1e-7 .. 4e-6 (fp32, cases 1-4 and 6), at most 9.6e-6 on case 5 in fp32 (36 % of the bar at worst) and
at 0.24 .. 0.39 of the bf16 bars.

Wrong kernels, each built as a CPU reference function (_manual(variant=...), _wrong) and measured against the right reference on the
cases meant to catch it (test_wrong_kernels_land_outside_the_bars_cpu asserts >= 10 x the bar, without a GPU; the figures are the bf16
ones, the distance of the worst-hit output and that distance over its bar -- in fp32 the bar is 2e-5 and the ratios are 1e4 .. 1e6):
  1  channels 64..127 of dq / dk / dv zero       dh 65: 0.50 / 0.59 / 0.66 (31 x / 49 x / 54 x); dh 80, 128, cross 128: 0.78 .. 1.0 (60 x .. 180 x)
  2  causal_off taken as 0                       case 3: 3.5 .. 4.9 (560 x, 590 x)
  3  dkdv start chunk: `lo` rounded up           case 1 causal, dh 16 / 128: dk 0.54 / 0.48 (55 x / 36 x)
     rows of chunk 0 staged at the start chunk   case 1 causal, dh 16 / 128: dk 22 / 5.3 (2300 x / 560 x)
     (both differ from the right kernel only where the start chunk is above 0: the sequences of 65, 130 and 200 rows)
  4  row strides taken as H * dh                 fused dh 80 / 128: 4.0 / 3.0 (290 x / 340 x)
  5  D_i omitted                                 0.23 .. 2.4 on dq, dk (34 x on case 3 .. 240 x); dv is unaffected
  6  scale in s only, not in ds                  sqrt(dh) - 1 on dq, dk: 7.9 (dh 80), 10.3 (dh 128), 7.0 (cross 64) (740 x .. 880 x); exactly
                                                 0 on the scale = 1.0 cases, which is why both kinds exist
  7  k and v swapped in pass B                   1.2 .. 9.0 (150 x .. 1200 x)
  8  softmax without the max subtraction         case 5, fp32 arithmetic: inf / NaN in every output"""
import ctypes
import functools

import pytest
import torch

gpu = pytest.mark.gpu

F32_BAR = 2e-5          # the project's fp32 bar (test_attention_bwd_vs_autograd, test_attention_f32, test_tp_neuron_ops_gpu.py)
BF16_CAP = 6e-2         # the bar of test_attention_bwd_vs_autograd in bf16: no derived bar may exceed it
AB_RB, AB_CH = 16, 64   # csrc/attention_bwd.hip: rows per workgroup, staged rows per chunk
LENS = [1, 15, 16, 17, 63, 64, 65, 130, 200]
DHS = [8, 16, 64, 65, 80, 88, 96, 128]
DTYPES = [torch.float32, torch.bfloat16]
OUT = ("dq", "dk", "dv")


@pytest.fixture(scope="module")
def L():
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    lib.load()
    return lib


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def _self_desc(lens, gaps=None, tail=0):
    """own-key descriptors of sequences packed along one row set, gaps[i] unowned rows in front of sequence i, `tail` behind the last"""
    desc, r = [], 0
    for i, n in enumerate(lens):
        r += gaps[i] if gaps else 0
        desc.append((r, n, 0, 0, r, n))
        r += n
    return desc, r + tail


def _cross_desc(qn, kn):
    """queries of one row set over keys of ANOTHER, named through the own-key fields (Blip2Engine.qformer_backward)"""
    desc, a, b = [], 0, 0
    for n, m in zip(qn, kn):
        desc.append((a, n, 0, 0, b, m))
        a, b = a + n, b + m
    return desc, a, b


@functools.lru_cache(maxsize=None)
def _spec(name):
    """geometry of one named case: desc, Rq / Rk (rows of the query / key row set; one fused q | k | v buffer when they are the same set),
    H, dh, scale, causal, gain (factor on q and k)"""
    s = dict(name=name, gain=1.0, cross=False, seed=17)
    part = name.split("_")
    if part[0] == "self":                        # self_dh<dh>_<causal|full>[_scale1]: case 1
        s.update(H=3, dh=int(part[1][2:]), causal=int(part[2] == "causal"))
        s["desc"], s["Rq"] = _self_desc(LENS)
        if part[-1] == "scale1":
            s["scale"] = 1.0
    elif part[0] == "cross":                     # case 2
        s.update(H=2, dh=int(part[1][2:]), causal=0, cross=True)
        s["desc"], s["Rq"], s["Rk"] = _cross_desc([32, 32, 5], [257, 70, 64])
    elif part[0] == "off":                       # case 3: causal, ko_len > q_len
        s.update(H=2, dh=int(part[1][2:]), causal=1, cross=True)
        s["desc"], s["Rq"], s["Rk"] = _cross_desc([5, 17, 64], [70, 17 + 64, 130])
    elif part[0] == "fused":                     # cases 4 (strides) and 6
        s.update(H=3, dh=int(part[1][2:]), causal=1)
        s["desc"], s["Rq"] = _self_desc([17, 65, 130])
    elif part[0] == "padded":                    # case 4: gaps of 1..7 unowned rows and one empty descriptor that points into a gap
        s.update(H=2, dh=80, causal=int(part[1] == "causal"))
        desc, s["Rq"] = _self_desc([5, 17, 64, 65, 130, 1], gaps=[3, 1, 7, 2, 5, 6], tail=4)
        s["desc"] = desc[:2] + [(desc[2][0] - 4, 0, 0, 0, desc[2][0] - 4, 0)] + desc[2:]
    elif part[0] == "qlen0":                     # case 4: keys without a query
        s.update(H=2, dh=65, causal=int(part[1] == "causal"))
        s["desc"], s["Rq"] = [(0, 20, 0, 0, 0, 20), (20, 0, 0, 0, 20, 30)], 50
    elif part[0] == "large":                     # case 5: scores of standard deviation ~32
        s.update(H=3, dh=80, causal=int(part[1] == "causal"), gain=32 ** 0.5)
        s["desc"], s["Rq"] = _self_desc([65, 130])
    elif part[0] == "prefix":                    # descriptors that name a visible prefix (kp_len != 0): the backward ignores it
        s.update(H=2, dh=80, causal=1, scale=1.0)
        s["desc"], s["Rq"] = [(0, 32, 0, 0, 0, 32), (32, 16, 0, 32, 32, 16), (48, 70, 0, 32, 48, 70)], 118
    else:
        raise KeyError(name)
    s.setdefault("scale", s["dh"] ** -0.5)
    s.setdefault("Rk", s["Rq"])
    s["max_len"] = max(max(d[1], d[5]) for d in s["desc"])
    return s


@functools.lru_cache(maxsize=None)
def _data(name, dtype):
    """operands of a case as fp32 CPU tensors that hold values of `dtype` (rounded before any reference sees them): q, k, v -- column
    views of one [R, 3 * H * dh] buffer `qkv` unless the case is cross attention -- and d_out"""
    s = _spec(name)
    g = torch.Generator().manual_seed(s["seed"] + s["dh"])
    d = s["H"] * s["dh"]
    rnd = lambda t: t.to(dtype).to(torch.float32)   # noqa: E731
    if s["cross"]:
        qkv = None
        q = rnd(s["gain"] * torch.randn(s["Rq"], d, generator=g))
        k = rnd(s["gain"] * torch.randn(s["Rk"], d, generator=g))
        v = rnd(torch.randn(s["Rk"], d, generator=g))
    else:
        qkv = torch.randn(s["Rq"], 3 * d, generator=g)
        qkv[:, :2 * d] *= s["gain"]
        qkv = rnd(qkv)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    go = rnd(torch.randn(s["Rq"], d, generator=g))
    return dict(q=q, k=k, v=v, go=go, qkv=qkv)


def _owned(s):
    """bool [Rq], [Rk]: rows that belong to some sequence"""
    oq, ok = torch.zeros(s["Rq"], dtype=torch.bool), torch.zeros(s["Rk"], dtype=torch.bool)
    for (qs, ql, _, _, ks, kl) in s["desc"]:
        oq[qs:qs + ql] = True
        ok[ks:ks + kl] = True
    return oq, ok


# ---------------------------------------------------------------------------------------------------------------------------------------
# references (CPU only)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _heads(t, start, n, H, dh):
    return t[start:start + n].reshape(n, H, dh).transpose(0, 1)          # [H, n, dh]


def _rows(t):
    return t.transpose(0, 1).reshape(t.shape[1], -1)                       # [H, n, dh] -> [n, H * dh]


def _mask(ql, kl, causal, off=None):
    """key j <= query i + (ko_len - q_len), the formula of _ref_attention in tests/test_ops_gpu.py"""
    if not causal:
        return None
    off = kl - ql if off is None else off
    return torch.arange(kl)[None, :] <= torch.arange(ql)[:, None] + off


def _scores(qq, kk, scale, m):
    sc = qq @ kk.transpose(1, 2) * scale
    return sc if m is None else sc.masked_fill(~m, float("-inf"))


def _forward(q, k, v, s, dtype=torch.float64):
    """plain attention of every sequence and head in `dtype`; rows of no sequence are 0"""
    H, dh = s["H"], s["dh"]
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    o = torch.zeros(s["Rq"], H * dh, dtype=dtype)
    for (qs, ql, _, _, ks, kl) in s["desc"]:
        if ql and kl:
            sc = _scores(_heads(q, qs, ql, H, dh), _heads(k, ks, kl, H, dh), s["scale"], _mask(ql, kl, s["causal"]))
            o[qs:qs + ql] = _rows(torch.softmax(sc, -1) @ _heads(v, ks, kl, H, dh))
    return o


def _autograd(q, k, v, go, s):
    """THE reference: float64 forward, torch.autograd gradient for d_out -> (o, dq, dk, dv), all float64"""
    leaves = [t.double().clone().requires_grad_(True) for t in (q, k, v)]
    o = _forward(*leaves, s)
    grads = torch.autograd.grad((o * go.double()).sum(), leaves, allow_unused=True)
    return (o.detach(),) + tuple(torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(grads, leaves))


def _dkdv_blocks(qq, kk, vv, gg, Lse, D, scale, off, mode):
    """dk / dv of one causal sequence the way attn_bwd_dkdv_kernel walks it -- per block of AB_RB keys, queries from a start chunk on --
    with the "right" start chunk or a WRONG one: "up" rounds the first visible query `lo` up to a chunk instead of down; "shift" stages the rows of chunk 0
    (q, d_out, statistics) while it counts queries from the start chunk"""
    ql, kl = qq.shape[1], kk.shape[1]
    dk, dv = torch.zeros_like(kk), torch.zeros_like(vv)
    for j0 in range(0, kl, AB_RB):
        j1 = min(j0 + AB_RB, kl)
        lo = max(0, j0 - off)
        if mode == "up":
            i = torch.arange(min(-(-lo // AB_CH) * AB_CH, ql), ql)
            src = i
        elif mode == "right":
            i = torch.arange(lo // AB_CH * AB_CH, ql)
            src = i
        else:
            i = torch.arange(lo // AB_CH * AB_CH, ql)
            src = i - lo // AB_CH * AB_CH
        if i.numel() == 0:
            continue
        m = torch.arange(j0, j1)[None, :] <= i[:, None] + off
        p = torch.exp(qq[:, src] @ kk[:, j0:j1].transpose(1, 2) * scale - Lse[:, src]) * m
        ds = p * (gg[:, src] @ vv[:, j0:j1].transpose(1, 2) - D[:, src])
        dk[:, j0:j1] = scale * ds.transpose(1, 2) @ qq[:, src]
        dv[:, j0:j1] = p.transpose(1, 2) @ gg[:, src]
    return dk, dv


def _manual(q, k, v, o, go, s, dtype=torch.float64, variant=None):
    """The kernel's formulas in plain PyTorch, `dtype` arithmetic: P = exp(s - L), D_i = d_out_i . o_i with the o GIVEN, dS = P (dP - D),
    dq = scale dS k, dk = scale dS^T q, dv = P^T d_out.  In float64 with the float64 o this is _autograd (test_reference_cpu).  It carries
    the bf16 / fp32 floors (an inexact o, fp32 arithmetic) and, through `variant`, the wrong kernels of the module docstring."""
    H, dh, scale = s["H"], s["dh"], s["scale"]
    q, k, v, o, go = (t.to(dtype) for t in (q, k, v, o, go))
    dq = torch.zeros(s["Rq"], H * dh, dtype=dtype)
    dk, dv = torch.zeros(s["Rk"], H * dh, dtype=dtype), torch.zeros(s["Rk"], H * dh, dtype=dtype)
    for (qs, ql, _, _, ks, kl) in s["desc"]:
        if not (ql and kl):
            continue
        qq, oo, gg = (_heads(t, qs, ql, H, dh) for t in (q, o, go))
        kk, vv = (_heads(t, ks, kl, H, dh) for t in (k, v))
        off = 0 if variant == "causal_off0" else kl - ql
        m = _mask(ql, kl, s["causal"], off)
        sc = _scores(qq, kk, scale, m)
        if variant == "no_max":                  # softmax without the running max: exp of the raw scores
            e = torch.exp(sc)
            Lse = torch.log(e.sum(-1, keepdim=True))
            P = e / e.sum(-1, keepdim=True)
        else:
            Lse = torch.logsumexp(sc, -1, keepdim=True)
            P = torch.exp(sc - Lse)
        D = torch.zeros_like(Lse) if variant == "no_D" else (gg * oo).sum(-1, keepdim=True)
        if variant == "swap_kv":                 # pass B stages v where k belongs and k where v belongs (both kernels)
            P = torch.exp(_scores(qq, vv, scale, m) - Lse)
            kk, vv = vv, kk
        dS = P * (gg @ vv.transpose(1, 2) - D)
        sc2 = 1.0 if variant == "scale_once" else scale       # scale in s only, not in ds
        dqh, dkh, dvh = sc2 * dS @ kk, sc2 * dS.transpose(1, 2) @ qq, P.transpose(1, 2) @ gg
        if variant in ("start_up", "start_shift", "start_right") and s["causal"]:
            dkh, dvh = _dkdv_blocks(qq, kk, vv, gg, Lse, D, scale, off, variant[6:])
        dq[qs:qs + ql], dk[ks:ks + kl], dv[ks:ks + kl] = _rows(dqh), _rows(dkh), _rows(dvh)
    if variant in ("zero_hi_dq", "zero_hi_dk", "zero_hi_dv"):            # the second accumulator (channels 64..127 of every head) is lost
        t = dict(zero_hi_dq=dq, zero_hi_dk=dk, zero_hi_dv=dv)[variant]
        t.view(-1, H, dh)[:, :, 64:] = 0
    return dq, dk, dv


def _as_if_ld_were_width(qkv, part, d):
    """what a kernel reads as q (part 0), k (1), v (2) of the fused buffer if it takes the row stride to be H * dh, not 3 * H * dh"""
    R = qkv.shape[0]
    return qkv.reshape(-1)[part * d + torch.arange(R)[:, None] * d + torch.arange(d)[None, :]]


def _dist(got, ref):
    """max |got - ref| / max |ref|, the project's metric; inf when `got` is not finite"""
    if not torch.isfinite(got).all():
        return float("inf")
    return ((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    """(o, dq, dk, dv) in float64 on the case's operands as rounded to `dtype`: computed once, shared, never modified"""
    c = _data(name, dtype)
    return _autograd(c["q"], c["k"], c["v"], c["go"], _spec(name))


@functools.lru_cache(maxsize=None)
def _floors(name, dtype):
    """What the reference alone says about the precision a correct kernel can have on this case, per output (dq, dk, dv):
      round : the float64 gradient rounded to bf16                                  (the kernel stores bf16)
      d_i   : the float64 gradient formulas with D_i taken from the bf16-rounded o  (the kernel is handed a bf16 o)
      f32   : the formulas evaluated in plain fp32 PyTorch, forward included        (the kernel's arithmetic is fp32)"""
    s, c = _spec(name), _data(name, dtype)
    o, *ref = _reference(name, dtype)
    fl = {}
    if dtype == torch.bfloat16:
        fl["round"] = [_dist(_bf(r), r) for r in ref]
        fl["d_i"] = [_dist(g, r) for g, r in zip(_manual(c["q"], c["k"], c["v"], _bf(o), c["go"], s), ref)]
    if name.startswith("large"):
        o32 = _forward(c["q"], c["k"], c["v"], s, torch.float32)
        fl["f32"] = [_dist(g, r) for g, r in zip(_manual(c["q"], c["k"], c["v"], o32, c["go"], s, torch.float32), ref)]
    return fl


@functools.lru_cache(maxsize=None)
def _bars(name, dtype):
    """fp32: 2e-5, the project's bar.  bf16: 4 x the larger floor, never above 6e-2.  The large-logit cases: 4 x the fp32-evaluation floor
    (in bf16: 4 x the largest of the three floors, never above 6e-2)."""
    fl = _floors(name, dtype)
    if not fl:
        return [F32_BAR] * 3
    bars = [4 * max(f[i] for f in fl.values()) for i in range(3)]
    return [min(b, BF16_CAP) for b in bars] if dtype == torch.bfloat16 else bars


def _mfma_forward_floor(name):
    """Case 6 in bf16: the forward as a bf16 MFMA kernel must compute it -- bf16 operands, fp32 scores and statistics, P rounded to bf16
    because it is an MFMA operand of P @ v, the normaliser unrounded, o stored in bf16 -- then the backward formulas in fp32 on that o and
    the gradients stored in bf16; distance from the float64 reference per output"""
    s, c = _spec(name), _data(name, torch.bfloat16)
    H, dh = s["H"], s["dh"]
    o = torch.zeros(s["Rq"], H * dh)
    for (qs, ql, _, _, ks, kl) in s["desc"]:
        sc = _scores(_heads(c["q"], qs, ql, H, dh), _heads(c["k"], ks, kl, H, dh), s["scale"], _mask(ql, kl, s["causal"]))
        p = torch.exp(sc - sc.max(-1, keepdim=True).values)
        o[qs:qs + ql] = _rows((_bf(p) @ _heads(c["v"], ks, kl, H, dh)) / p.sum(-1, keepdim=True))
    got = _manual(c["q"], c["k"], c["v"], _bf(o), c["go"], s, torch.float32)
    return [_dist(_bf(g), r) for g, r in zip(got, _reference(name, torch.bfloat16)[1:])]


# ---------------------------------------------------------------------------------------------------------------------------------------
# wrong kernels (module docstring): variant, the cases meant to catch it
# ---------------------------------------------------------------------------------------------------------------------------------------
WRONG = [
    ("zero_hi_dq", ["self_dh65_causal", "self_dh80_full", "self_dh128_causal", "cross_dh128"]),
    ("zero_hi_dk", ["self_dh65_causal", "self_dh80_full", "self_dh128_causal", "cross_dh128"]),
    ("zero_hi_dv", ["self_dh65_causal", "self_dh80_full", "self_dh128_causal", "cross_dh128"]),
    ("causal_off0", ["off_dh16", "off_dh128"]),
    ("start_up", ["self_dh16_causal", "self_dh128_causal"]),
    ("start_shift", ["self_dh16_causal", "self_dh128_causal"]),
    ("ld_width", ["fused_dh80", "fused_dh128"]),
    ("no_D", ["self_dh16_causal", "self_dh128_full", "cross_dh64", "off_dh128"]),
    ("scale_once", ["self_dh80_causal", "self_dh128_full", "cross_dh64"]),
    ("swap_kv", ["self_dh16_causal", "self_dh128_full", "cross_dh64"]),
    ("no_max", ["large_causal", "large_full"]),
]


def _wrong(variant, name, dtype):
    """per output, the distance of the wrong kernel `variant` from the reference of the case"""
    s, c = _spec(name), _data(name, dtype)
    o, *ref = _reference(name, dtype)
    q, k, v = c["q"], c["k"], c["v"]
    if variant == "ld_width":
        d = s["H"] * s["dh"]
        q, k, v = (_as_if_ld_were_width(c["qkv"], i, d) for i in range(3))
        variant = None
    if variant == "no_max":       # what overflows is fp32 arithmetic
        got = _manual(q, k, v, o, c["go"], s, torch.float32, variant)
    else:
        got = _manual(q, k, v, o, c["go"], s, torch.float64, variant)
    return [_dist(g, r) for g, r in zip(got, ref)]


def test_reference_cpu():
    """No GPU.  The hand-written backward formulas that carry the floors and the wrong variants ARE the autograd reference when nothing is
    wrong with them (float64, exact o): 1e-12 on one case of every kind."""
    for name in ("self_dh65_causal", "self_dh80_full_scale1", "cross_dh64", "off_dh16", "padded_causal", "qlen0_causal", "large_causal"):
        s, c = _spec(name), _data(name, torch.float32)
        o, *ref = _reference(name, torch.float32)
        for g, r in zip(_manual(c["q"], c["k"], c["v"], o, c["go"], s), ref):
            assert _dist(g, r) < 1e-12, name
        if s["causal"]:     # ... and the block-wise dk / dv walk of the wrong-start variants, given the RIGHT start chunk, is the plain sum
            for g, r in zip(_manual(c["q"], c["k"], c["v"], o, c["go"], s, variant="start_right"), ref):
                assert _dist(g, r) < 1e-12, name


@pytest.mark.parametrize("variant,names", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_kernels_land_outside_the_bars_cpu(variant, names):
    """No GPU.  Every wrong kernel of the module docstring, built as a CPU reference function, lands at least 10 x the bar away from the
    right reference on the cases meant to catch it, on at least one output (the outputs it leaves right are 0 away), in both dtypes."""
    for name in names:
        for dtype in DTYPES:
            dist, bars = _wrong(variant, name, dtype), _bars(name, dtype)
            ratio = max(d_ / b for d_, b in zip(dist, bars))
            print("%-12s %-18s %-8s dist %s  bars %s  worst / bar %.3g" % (variant, name, str(dtype)[6:], _fmt(dist), _fmt(bars), ratio))
            assert ratio >= 10, (variant, name, dtype, dist, bars)


def test_large_logit_case_is_large_cpu():
    """No GPU.  Case 5 is what it says: scores of standard deviation ~30, row maxima around 100 -- above 88.7, where exp overflows fp32, on
    many rows -- and far below fp32 overflow of the scores themselves."""
    for name in ("large_causal", "large_full"):
        s, c = _spec(name), _data(name, torch.float32)
        H, dh = s["H"], s["dh"]
        for (qs, ql, _, _, ks, kl) in s["desc"]:
            sc = _heads(c["q"].double(), qs, ql, H, dh) @ _heads(c["k"].double(), ks, kl, H, dh).transpose(1, 2) * s["scale"]
            assert 25 < sc.std().item() < 40
            mx = _scores(_heads(c["q"].double(), qs, ql, H, dh), _heads(c["k"].double(), ks, kl, H, dh), s["scale"],
                         _mask(ql, kl, s["causal"])).max(-1).values
            assert (mx > 89).sum().item() >= 16 and mx.max().item() < 300


def _fmt(x):
    return "(" + ", ".join("%.3g" % v for v in x) + ")"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def _dev(t, dtype):
    return t.to(dtype).to("cuda")


def _desc_dev(s):
    return torch.tensor(s["desc"], dtype=torch.int32, device="cuda")


def _operands(name, dtype, fused=False):
    """device q, k, v (contiguous, or column views of the fused buffer), o = the reference output rounded to dtype, d_out"""
    c = _data(name, dtype)
    if fused:
        d = _spec(name)["H"] * _spec(name)["dh"]
        qkv = _dev(c["qkv"], dtype)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        assert q.stride(0) == 3 * d and not k.is_contiguous()
    else:
        q, k, v = (_dev(c[x].contiguous(), dtype) for x in "qkv")
    return q, k, v, _dev(_reference(name, dtype)[0], dtype), _dev(c["go"], dtype)


def _bwd(L, name, q, k, v, o, go):
    s = _spec(name)
    return L.attention_bwd(q, k, v, o, go, _desc_dev(s), len(s["desc"]), s["max_len"], s["H"], s["dh"], s["scale"], s["causal"])


def _check(tag, got, ref, bars):
    errs = [_dist(g.cpu(), r) for g, r in zip(got, ref)]
    print("%s: max |err| / max |ref| (dq, dk, dv) %s  bars %s" % (tag, _fmt(errs), _fmt(bars)))
    for n, g, r, e, b in zip(OUT, got, ref, errs, bars):
        assert g.shape == r.shape and torch.isfinite(g).all(), (tag, n)
        assert e < b, (tag, n, e, b)


def _run_case(L, name, dtype, fused=False):
    got = _bwd(L, name, *_operands(name, dtype, fused))
    assert all(g.dtype == dtype for g in got)
    _check("%s %s" % (name, str(dtype)[6:]), got, _reference(name, dtype)[1:], _bars(name, dtype))
    return got


CASE1 = ["self_dh%d_%s" % (dh, m) for dh in DHS for m in ("causal", "full")] + ["self_dh80_causal_scale1", "self_dh80_full_scale1"]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", CASE1)
def test_head_dims(L, name, dtype):
    """Case 1: every head dim, sequences of 1 .. 200 rows in one call (one to four chunks, dkdv start chunks 0, 64 and 128), causal and full"""
    _run_case(L, name, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["cross_dh64", "cross_dh128"])
def test_cross_attention(L, name, dtype):
    """Case 2: 32 / 32 / 5 queries over 257 / 70 / 64 keys of another row set; key blocks past the last query block and the reverse"""
    _run_case(L, name, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["off_dh16", "off_dh128"])
def test_causal_offset(L, name, dtype):
    """Case 3: causal with ko_len > q_len, (5, 70), (17, 81), (64, 130): key j is visible to query i when j <= i + ko_len - q_len"""
    _run_case(L, name, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["fused_dh80", "fused_dh128"])
def test_fused_qkv_views(L, name, dtype):
    """Case 4: q, k, v as column views of one [R, 3 * H * dh] buffer (every production caller): within the bar, and the same bits as the
    call on contiguous copies"""
    got = _run_case(L, name, dtype, fused=True)
    q, k, v, o, go = _operands(name, dtype, fused=True)
    again = _bwd(L, name, q.contiguous(), k.contiguous(), v.contiguous(), o, go)
    for n, a, b in zip(OUT, got, again):
        assert torch.equal(a, b), n


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["padded_causal", "padded_full"])
def test_padded_pack(L, name, dtype):
    """Case 4: gaps of 1..7 rows that belong to no sequence, NaN in every operand there, and one descriptor with q_len == ko_len == 0:
    sequence rows match the reference, gap rows of dq / dk / dv are exactly zero"""
    s = _spec(name)
    oq, ok = _owned(s)
    assert (~oq).sum() == 28 and torch.equal(oq, ok)
    q, k, v, o, go = _operands(name, dtype)
    for t in (q, k, v, o, go):
        t[~oq.to("cuda")] = float("nan")
    got = _bwd(L, name, q, k, v, o, go)
    _check("%s %s" % (name, str(dtype)[6:]), got, _reference(name, dtype)[1:], _bars(name, dtype))
    for n, g in zip(OUT, got):
        assert (g.cpu()[~oq] == 0).all(), n


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["qlen0_causal", "qlen0_full"])
def test_keys_without_queries(L, name, dtype):
    """Case 4: a descriptor with q_len == 0, ko_len > 0: dk and dv of its keys are exactly zero, the other sequence is untouched by it"""
    got = _run_case(L, name, dtype)
    assert (got[1][20:] == 0).all() and (got[2][20:] == 0).all() and (got[0][20:] == 0).all()


def _raw_call(L, dtype, s, q, k, v, o, go, dq, dk, dv, dh=None):
    fn = L.load().devqa_attention_bwd if dtype == torch.bfloat16 else L.load().devqa_attention_bwd_f32
    stats = torch.empty(s["Rq"] * s["H"] * 2, dtype=torch.float32, device="cuda")
    desc = _desc_dev(s)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = fn(p(q), q.stride(0), p(k), k.stride(0), p(v), v.stride(0), p(o), o.stride(0), p(go), go.stride(0), p(dq), dq.stride(0),
            p(dk), dk.stride(0), p(dv), dv.stride(0), p(stats), p(desc), len(s["desc"]), s["max_len"], s["H"],
            s["dh"] if dh is None else dh, s["scale"], s["causal"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


SENTINEL = -7.0


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_output_strides(L, dtype):
    """Case 4: the lddq / lddk / lddv of the C ABI.  dq | dk | dv are column views of one [R + 2, 3 * H * dh + 8] buffer full of a sentinel;
    after the call the first and last buffer row, the 8 spare columns and every row of no sequence still hold it, the rest is the reference"""
    name = "padded_causal"
    s = _spec(name)
    d, R = s["H"] * s["dh"], s["Rq"]
    oq, _ = _owned(s)
    q, k, v, o, go = _operands(name, dtype, fused=True)
    buf = torch.full((R + 2, 3 * d + 8), SENTINEL, dtype=dtype, device="cuda")
    outs = [buf[1:R + 1, i * d:(i + 1) * d] for i in range(3)]
    assert _raw_call(L, dtype, s, q, k, v, o, go, *outs) == 0
    _check("strided outputs %s" % str(dtype)[6:], [torch.where(oq.to("cuda")[:, None], t, torch.zeros_like(t)) for t in outs],
           _reference(name, dtype)[1:], _bars(name, dtype))
    rest = buf.clone()
    for t in (rest[1:R + 1, i * d:(i + 1) * d] for i in range(3)):
        t[oq.to("cuda")] = SENTINEL
    assert (rest == SENTINEL).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_two_calls_same_bits(L, dtype):
    """Case 4: the kernels use no atomics -- two identical calls give the same bits"""
    for name in ("self_dh80_causal", "cross_dh128"):
        ops = _operands(name, dtype)
        a, b = _bwd(L, name, *ops), _bwd(L, name, *ops)
        for n, x, y in zip(OUT, a, b):
            assert torch.equal(x, y), (name, n)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["large_causal", "large_full"])
def test_large_logits(L, name, dtype):
    """Case 5: scores of standard deviation ~32, row maxima around 100: finite, and within 4 x the floor of a plain fp32 evaluation"""
    _run_case(L, name, dtype, fused=True)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["fused_dh80", "fused_dh128"])
def test_forward_then_backward(L, name, dtype):
    """Case 6: as production runs it -- o comes from lib.attention on the same fused operands (the MFMA kernel in bf16, devqa_attention_f32
    in fp32), not from the reference; the reference stays float64 end to end"""
    s = _spec(name)
    q, k, v, _, go = _operands(name, dtype, fused=True)
    o = L.attention(q, k, v, _desc_dev(s), len(s["desc"]), max(d[1] for d in s["desc"]), s["H"], s["dh"], s["scale"], s["causal"])
    assert o.dtype == dtype
    if dtype == torch.bfloat16:
        floor = _mfma_forward_floor(name)
        bars = [min(4 * f, BF16_CAP) for f in floor]
        print("%s: bf16 forward-then-backward floor %s" % (name, _fmt(floor)))
    else:
        bars = [F32_BAR] * 3
    _check("fwd+bwd %s %s" % (name, str(dtype)[6:]), _bwd(L, name, q, k, v, o, go), _reference(name, dtype)[1:], bars)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("dh", [129, 0])
def test_bad_head_dim_is_refused_before_any_launch(L, dh, dtype):
    """Case 7: dh = 129 and dh = 0 are refused with the shape code (DEVQA_E_SHAPE, -2) and nothing is launched: outputs filled by the test
    keep their contents"""
    name = "qlen0_full"
    s = _spec(name)
    q, k, v, o, go = _operands(name, dtype)
    outs = [torch.full_like(q, SENTINEL) for _ in range(3)]
    assert _raw_call(L, dtype, s, q, k, v, o, go, *outs, dh=dh) == -2
    assert b"dh" in L.load().devqa_last_error()
    assert all((t == SENTINEL).all() for t in outs)
    wide = [torch.zeros(s["Rq"], s["H"] * max(dh, 1), dtype=dtype, device="cuda") for _ in range(5)]
    with pytest.raises(L.DevqaError, match=r"\(-2\)"):
        L.attention_bwd(*wide, _desc_dev(s), len(s["desc"]), s["max_len"], s["H"], dh, s["scale"], s["causal"])


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_visible_prefix_is_ignored(L, dtype):
    """Pins the documented behaviour: the backward supports the own-key part of a descriptor only.  For descriptors that name a visible
    prefix (kp_len != 0, what lib.attention honours) dq, dk and dv are the gradients of attention over the OWN keys alone: the prefix
    keys receive no gradient from those queries and dq has no term from them.  No caller in the package hands it such a descriptor."""
    name = "prefix_pin"
    assert any(d[3] for d in _spec(name)["desc"])
    _run_case(L, name, dtype)


if __name__ == "__main__":   # the floors, bars and wrong-kernel distances of the module docstring; needs no GPU
    for dt in DTYPES[::-1]:
        for nm in CASE1 + ["cross_dh64", "cross_dh128", "off_dh16", "off_dh128", "fused_dh80", "fused_dh128", "padded_causal", "padded_full",
                           "qlen0_causal", "qlen0_full", "large_causal", "large_full", "prefix_pin"]:
            fl = _floors(nm, dt)
            if fl:
                print("%-24s %-8s %s  bars %s" % (nm, str(dt)[6:], "  ".join("%s %s" % (k_, _fmt(v_)) for k_, v_ in fl.items()),
                                                 _fmt(_bars(nm, dt))))
    for nm in ("fused_dh80", "fused_dh128"):
        f6 = _mfma_forward_floor(nm)
        print("%-24s bf16 forward-then-backward floor %s  bars %s" % (nm, _fmt(f6), _fmt([min(4 * f, BF16_CAP) for f in f6])))
    for var, names in WRONG:
        for nm in names:
            for dt in DTYPES:
                dist, bars = _wrong(var, nm, dt), _bars(nm, dt)
                print("%-12s %-18s %-8s dist %s  worst / bar %.3g" % (var, nm, str(dt)[6:], _fmt(dist),
                                                                       max(d_ / b for d_, b in zip(dist, bars))))
