"""Op-level parity of the sentence encoder's own kernels (csrc/text_ops.hip: devqa_text_embed_ln / _f32, devqa_seq_pool) and of its bf16
attention call (devqa_attention on the fused q|k|v buffer) against float64 restatements on the CPU, on the operand values the kernel sees
(bf16 tables / operands rounded first).

Bars (the neighbouring op tests'): fp32 outputs atol 2e-5 / rtol 1e-5 (test_layernorm_fwd_bwd); a bf16 output next to an fp32 output of
the same call is that fp32 output cast, bit for bit (test_gelu_forward_and_backward).

Wrong variants of the float64 references, and how far each is from the right one on these inputs (max |diff| over the test's cases,
computed on the CPU; the outputs are O(1), the allowance is 2e-5 + 1e-5 |ref|):
  _embed_ln_ref without the token-type row                      2.4      test_embed_ln (both scales)
  _embed_ln_ref with eps 1e-5 instead of 1e-12                   2.3      test_embed_ln, scale 1e-3 (row variance 3e-6); 8e-6 at scale 1: invisible
  _embed_ln_ref with pos[r] = r instead of the given positions   3.8      test_embed_ln
  _pool_ref mean over the len - 2 inner rows (no specials)       0.06     test_seq_pool (mean)
  _pool_ref max started from 0 instead of -inf                   2.3      test_seq_pool (max: every input is negative)
The all-zero sequence has no wrong reference: it tells 0 from NaN (0 / 0 without the clamp of the norm)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD = dict(atol=2e-5, rtol=1e-5)


@pytest.fixture(scope="module")
def L():
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    lib.load()
    return lib


def dev(t):
    return t.to("cuda")


# ---------------------------------------------------------------------------------------------------------------------------------------
# embedding + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------------
V, P = 53, 128


def _embed_ln_ref(tok, pos, word, position, type0, g, b, eps, no_type=False):
    """float64 BertEmbeddings: LN(word[token] + type0 + position[pos])"""
    e = word.double()[tok.long()] + position.double()[pos.long()] + (0 if no_type else type0.double())
    m = e.mean(-1, keepdim=True)
    v = ((e - m) ** 2).mean(-1, keepdim=True)
    return (e - m) / torch.sqrt(v + eps) * g.double() + b.double()


def _embed_inputs(R, D, scale, dtype):
    gen = torch.Generator().manual_seed(1000 * D + R)
    word, position, type0 = (scale * torch.randn(s, generator=gen) for s in ((V, D), (P, D), (D,)))
    word, position, type0 = (t.to(dtype) for t in (word, position, type0))          # the values the kernel reads
    g, b = 1 + 0.1 * torch.randn(D, generator=gen), 0.1 * torch.randn(D, generator=gen)
    tok = torch.randint(0, V, (R,), generator=gen, dtype=torch.int32)
    pos = torch.randint(0, P, (R,), generator=gen, dtype=torch.int32)
    tok[0], pos[0] = V - 1, P - 1                     # the last row of either table
    if R > 2:
        tok[1], pos[1] = 0, 0
        tok[2], pos[2] = V - 1, 0
    return tok, pos, word, position, type0, g, b


# D 48: the tiny model (12 of a wave's 64 lanes hold a piece); 384: MiniLM (two pieces per lane, the second half empty); R 1: one live wave
# of a workgroup; 67: 17 workgroups, the last with 3 of 4 rows.  scale 1e-3: every row's variance is ~3e-6, where eps 1e-12 and 1e-5 differ
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("scale", [1.0, 1e-3])
@pytest.mark.parametrize("R", [1, 67])
@pytest.mark.parametrize("D", [48, 384])
def test_embed_ln(L, D, R, scale, dtype):
    tok, pos, word, position, type0, g, b = _embed_inputs(R, D, scale, dtype)
    ref = _embed_ln_ref(tok, pos, word, position, type0, g, b, 1e-12)
    args = [dev(t) for t in (tok, pos, word, position, type0, g, b)]
    ob, of = L.text_embed_ln(*args, 1e-12, want="both")
    torch.testing.assert_close(of.cpu().double(), ref, **FWD)
    assert torch.equal(ob, of.to(torch.bfloat16))
    only_f = L.text_embed_ln(*args, 1e-12, want="f32")
    only_b = L.text_embed_ln(*args, 1e-12, want="bf16")
    assert torch.equal(only_f, of) and torch.equal(only_b, ob)


def test_embed_ln_wide_rows(L):
    """D 4096 fills all 16 register pieces of a lane; 1028 leaves one live lane in the fifth piece (the 8-piece kernel)"""
    for D in (4096, 1028):
        tok, pos, word, position, type0, g, b = _embed_inputs(5, D, 1.0, torch.float32)
        ref = _embed_ln_ref(tok, pos, word, position, type0, g, b, 1e-12)
        of = L.text_embed_ln(*[dev(t) for t in (tok, pos, word, position, type0, g, b)], 1e-12, want="f32")
        torch.testing.assert_close(of.cpu().double(), ref, **FWD)


# ---------------------------------------------------------------------------------------------------------------------------------------
# sentence pooling
# ---------------------------------------------------------------------------------------------------------------------------------------
LENS = [65, 1, 128, 2, 64, 7, 63]        # 7: the all-zero sequence


def _pool_ref(x, starts, lens, mode, normalize):
    out = []
    for s, n in zip(starts, lens):
        r = x[s:s + n].double()
        e = r.sum(0) / max(float(n), 1e-9) if mode == "mean" else (r[0] if mode == "cls" else r.max(0).values)
        if normalize:
            e = e / e.norm().clamp_min(1e-12)
        out.append(e)
    return torch.stack(out)


def _pool_inputs(D, negative):
    gen = torch.Generator().manual_seed(D)
    gap = 3                                                # unused rows between sequences; the descriptors are not in row order either
    order = [2, 0, 5, 1, 6, 3, 4]
    starts, r = [0] * len(LENS), 0
    for i in order:
        starts[i] = r
        r += LENS[i] + gap
    x = torch.randn(r, D, generator=gen) + 0.3
    if negative:
        x = -x.abs() - 0.1
    x[starts[5]:starts[5] + LENS[5]] = 0
    return x, starts


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("mode", ["mean", "cls", "max"])
@pytest.mark.parametrize("D", [48, 384])
def test_seq_pool(L, D, mode, normalize):
    x, starts = _pool_inputs(D, negative=(mode == "max"))
    ref = _pool_ref(x, starts, LENS, mode, normalize)
    xd = dev(x)
    sd, ld = dev(torch.tensor(starts, dtype=torch.int32)), dev(torch.tensor(LENS, dtype=torch.int32))
    code = {"mean": L.POOL_MEAN, "cls": L.POOL_CLS, "max": L.POOL_MAX}[mode]
    out = L.seq_pool(xd, sd, ld, code, normalize)
    again = L.seq_pool(xd, sd, ld, code, normalize)
    assert torch.equal(out, again)                                    # fixed summation order: the same bits
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.cpu().double(), ref, **FWD)
    assert torch.equal(out[5], torch.zeros_like(out[5]))              # the all-zero sequence: zeros, not NaN, also when normalised
    if mode == "max":
        assert (out[[0, 1, 2, 3, 4, 6]] < 0).all()
    if normalize:
        n = out.double().norm(dim=1).cpu()
        assert torch.allclose(n[[0, 1, 2, 3, 4, 6]], torch.ones(6, dtype=torch.float64), atol=1e-6)


def test_seq_pool_wide_and_bounds(L):
    """D 1028: a thread's second column group (257 groups over 256 threads); a descriptor that runs past R reads only the rows below R, an
    empty sequence gives zeros (mean, cls) / -inf (max)"""
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(10, 1028, generator=gen)
    starts, lens = [0, 4, 6, 10], [4, 2, 9, 0]
    xd = dev(x)
    sd, ld = dev(torch.tensor(starts, dtype=torch.int32)), dev(torch.tensor(lens, dtype=torch.int32))
    out = L.seq_pool(xd, sd, ld, L.POOL_MEAN, True).cpu().double()
    ref = _pool_ref(x, [0, 4, 6], [4, 2, 4], "mean", True)
    torch.testing.assert_close(out[:3], ref, **FWD)
    assert torch.equal(out[3], torch.zeros(1028, dtype=torch.float64))
    assert torch.equal(L.seq_pool(xd, sd, ld, L.POOL_CLS, False)[3].cpu(), torch.zeros(1028))
    assert torch.isinf(L.seq_pool(xd, sd, ld, L.POOL_MAX, False)[3]).all()
    # an empty sequence is not rescaled: -inf stays -inf under normalize (not -inf * 0 = NaN), the other rows are normalised as usual
    mx = L.seq_pool(xd, sd, ld, L.POOL_MAX, True).cpu()
    assert torch.isinf(mx[3]).all() and (mx[3] < 0).all() and not torch.isnan(mx).any()
    torch.testing.assert_close(mx[:3].double(), _pool_ref(x, [0, 4, 6], [4, 2, 4], "max", True), **FWD)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the encoder's bf16 attention call: lib.attention on the fused q|k|v buffer, read in place
# ---------------------------------------------------------------------------------------------------------------------------------------
ATT_LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]      # around every 16-row fragment, the 64-key chunk and the 64-query tile


def _att_ref(qkv, lens, H, dh, scale_exp=-0.5, causal=False):
    """float64 softmax(q k^T dh^-0.5) v per (sequence, head) on the bf16 operand values"""
    x = qkv.double()
    D = H * dh
    out = torch.empty(x.shape[0], D, dtype=torch.float64)
    r0 = 0
    for n in lens:
        for h in range(H):
            q, k, v = (x[r0:r0 + n, o * D + h * dh:o * D + (h + 1) * dh] for o in range(3))
            s = q @ k.T * dh ** scale_exp
            if causal:
                s = s.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), float("-inf"))
            out[r0:r0 + n, h * dh:(h + 1) * dh] = torch.softmax(s, -1) @ v
        r0 += n
    return out


def _att_inputs(H, dh):
    gen = torch.Generator().manual_seed(100 * H + dh)
    R = sum(ATT_LENS)
    qkv = torch.randn(R, 3 * H * dh, generator=gen)
    qkv[:, :2 * H * dh] *= 2 ** 0.5          # q, k ~ N(0, 2): logits q.k dh^-0.5 ~ N(0, 4), the largest of a 128 x 128 block about +-8
    return qkv.to(torch.bfloat16)


@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("dh", [16, 32, 64])
def test_attention_on_packed_sentences(L, dh, H):
    """lib.attention as SentenceEncoder calls it in bf16 mode: 13 packed sentences of 1..128 rows in one call, q | k | v views of the fused
    buffer with row stride 3 H dh, one descriptor per sentence, the self_full promise, scale dh^-0.5, logits up to about +-8; against float64
    softmax attention at the README's bf16 bar (1e-2 of the tensor's scale).
    Wrong variants of _att_ref on these inputs (max |diff| / max |ref|, CPU): scale dh^-1 instead of dh^-0.5 0.77..1.0; causal instead of
    full 1.1..1.7 over the nine cases; the largest |logit| of the 128-row sentence is 8.3..9.7."""
    qkv = _att_inputs(H, dh)
    ref = _att_ref(qkv, ATT_LENS, H, dh)
    D = H * dh
    d = dev(qkv)
    starts = [sum(ATT_LENS[:i]) for i in range(len(ATT_LENS))]
    desc = dev(torch.tensor([[s, n, 0, 0, s, n] for s, n in zip(starts, ATT_LENS)], dtype=torch.int32))
    q, k, v = d[:, :D], d[:, D:2 * D], d[:, 2 * D:]
    assert q.stride(0) == 3 * D and not k.is_contiguous()
    out = L.attention(q, k, v, desc, len(ATT_LENS), max(ATT_LENS), H, dh, dh ** -0.5, 0, self_full=True)
    assert out.shape == (sum(ATT_LENS), D) and out.dtype == torch.bfloat16 and torch.isfinite(out).all()
    err = ((out.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    print("attention dh %d H %d: rel err %.3g" % (dh, H, err))
    assert err < 1e-2
    assert torch.equal(d, dev(qkv))                                   # read in place: the fused buffer is untouched
