"""GPU: the seam between the frozen decoder prefix and stage B of the batched FT_VL evaluation.

1. devqa_llm_prefix_rows: the last decoder layer runs everything behind its attention on the KEPT rows alone.  The kept rows must
   equal the same rows of the all-rows call (devqa_llm_layers_ex, stop_before_fc2 = 1) BIT FOR BIT in both compute modes, on the tiny
   BLIP-2 / LLaVA models and on one decoder layer at the OPT-2.7B per-layer dims, where the kept-row GEMMs would by themselves take
   another kernel family or split-K slicing than the all-rows call; x is left holding the residual stream before the last layer.
2. The grouped post-edit tail (devqa_gather_cols_grouped + devqa_gemm_grouped: two launches for all cycles) against the per-edit loop
   of lib.gather_cols + lib.gemm it replaces, bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. kept rows of the last layer
# ---------------------------------------------------------------------------------------------------------------------------------
def _tiny_blip2(gold_dir, mode):
    import devqa_amd  # noqa: F401
    from devqa_amd.editor.vllms_for_edit.blip2.blip2 import BLIP2OPTForEdit
    vllm = BLIP2OPTForEdit(os.path.join(gold_dir, "tiny_blip2"), "cuda:0", dtype=mode)
    seqs = [(0, [2, 17, 33, 21, 9]), (0, [2, 5, 6]), (1, [2, 8, 9, 10, 11, 12, 13]), (None, [2, 4, 5, 6, 7])]
    return vllm.engine, seqs


def _tiny_llava(gold_dir, mode):
    import devqa_amd  # noqa: F401
    from devqa_amd.editor.vllms_for_edit.llava.llava import LlavaForEdit
    vllm = LlavaForEdit(os.path.join(gold_dir, "tiny_llava"), "cuda:0", True, dtype=mode)
    eng = vllm.engine
    im = eng.image_token_id
    ids = [t for t in range(3, 40) if t != im]
    seqs = [(0, [1, im] + ids[:4]), (0, [1, im] + ids[4:7]), (1, [1, im] + ids[7:14]), (None, [1] + ids[14:18])]
    return eng, seqs


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("family", ["blip2", "llava"])
def test_kept_rows_equal_all_rows_on_the_tiny_models(gold_dir, family, mode):
    eng, seqs = (_tiny_blip2 if family == "blip2" else _tiny_llava)(gold_dir, mode)
    assert eng.path_ctx() is not None
    g = torch.Generator().manual_seed(11)
    img_tokens = (torch.randn(2, eng.Q, eng.t["hidden_size"], generator=g) * 0.5).cuda()
    last = eng.t["num_hidden_layers"] - 1

    def pack():
        return eng.pack_from_tokens(seqs, img_tokens, share_prefix=True)
    ps = pack()
    x_all, a_all = eng.decoder_layers(ps, stop_before_fc2=True)
    R = x_all.shape[0]
    ps = pack()
    x_prev, _ = eng.decoder_layers(ps, upto_layer=last - 1)
    first_text, two_label = ps.start[0], [ps.start[1] + ps.length[1] - 2, ps.start[1] + ps.length[1] - 1]
    for keep in ([R // 2], sorted(r for r in {first_text, R - 1, *two_label, 3, R // 3} if 0 <= r < R), list(range(R))):
        ps = pack()
        xk, ak = eng.decoder_layers(ps, stop_before_fc2=True, keep_rows=keep)
        kd = torch.tensor(keep, device="cuda")
        assert xk.shape == (len(keep), x_all.shape[1]) and ak.shape == (len(keep), a_all.shape[1]) and ak.dtype == a_all.dtype
        assert torch.equal(xk, x_all[kd]), (family, mode, len(keep))
        assert torch.equal(ak, a_all[kd]), (family, mode, len(keep))
        assert torch.equal(ps.x, x_prev)            # the residual stream BEFORE the last layer
    # the Python-ordered cross-check schedule returns the same compact buffers
    keep = sorted({first_text, R - 1, *two_label})
    os.environ["DEVQA_PATH_ABI"] = "0"
    try:
        assert eng.path_ctx() is None
        xk, ak = eng.decoder_layers(pack(), stop_before_fc2=True, keep_rows=keep)
    finally:
        del os.environ["DEVQA_PATH_ABI"]
    kd = torch.tensor(keep, device="cuda")
    assert torch.equal(xk, x_all[kd]) and torch.equal(ak, a_all[kd])


D_OPT, F_OPT, H_OPT, Q_OPT, R_OPT = 2560, 10240, 32, 32, 600
TEXT_LENS = [130, 97, 141, 88, 80]          # 2 x 32 prefix rows + 536 text rows = 600: no multiple of 128 or 256


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def opt_layer(request):
    """ONE decoder layer at the OPT-2.7B per-layer dims behind a path-level context of its own, a shared-prefix pack of two image
    prefixes and five text sequences (the last one text-only), and the all-rows call's products (computed once, left unchanged)."""
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    mode = request.param
    adt = torch.bfloat16 if mode == "bf16" else torch.float32
    g = torch.Generator().manual_seed(23)
    D, F = D_OPT, F_OPT
    p = "language_model.model.decoder.layers.0."

    def mat(n, k, s):
        return (torch.randn(n, k, generator=g) * s).to(adt).cuda().contiguous()

    def vec(n, s, base=0.0):
        return (base + torch.randn(n, generator=g) * s).cuda().contiguous()
    w = {p + "self_attn_layer_norm.weight": vec(D, 0.1, 1.0), p + "self_attn_layer_norm.bias": vec(D, 0.05),
         "derived.dec_qkv.0.weight": mat(3 * D, D, 0.02), "derived.dec_qkv.0.bias": vec(3 * D, 0.02),
         p + "self_attn.out_proj.weight": mat(D, D, 0.02), p + "self_attn.out_proj.bias": vec(D, 0.02),
         p + "final_layer_norm.weight": vec(D, 0.1, 1.0), p + "final_layer_norm.bias": vec(D, 0.05),
         p + "fc1.weight": mat(F, D, 0.02), p + "fc1.bias": vec(F, 0.02)}
    desc = lib.ModelDesc(family=lib.FAMILY_BLIP2_OPT, compute_dtype=lib.DTYPE_BF16 if mode == "bf16" else lib.DTYPE_F32, image_size=28, patch_size=14,
                         v_hidden=64, v_layers=1, v_heads=4, v_ffn=128, q_hidden=64, q_layers=1, q_heads=4, q_ffn=128, q_cross_freq=1,
                         num_query_tokens=Q_OPT, t_hidden=D, t_layers=1, t_heads=H_OPT, t_ffn=F, t_vocab=50272, t_max_pos=2048, v_ln_eps=1e-5,
                         q_ln_eps=1e-12, t_ln_eps=1e-5)
    ctx = lib.PathContext(0, desc, w)
    rows, r, spans = [], 0, []
    for _ in range(2):
        rows.append([r, Q_OPT, 0, 0, r, Q_OPT])
        r += Q_OPT
    for i, n in enumerate(TEXT_LENS):
        rows.append([r, n, (i % 2) * Q_OPT, Q_OPT, r, n] if i < 4 else [r, n, 0, 0, r, n])
        spans.append((r, n))
        r += n
    assert r == R_OPT
    sd = torch.tensor(rows, dtype=torch.int32, device="cuda")
    x0 = torch.randn(R_OPT, D, generator=g).cuda()
    x_all = x0.clone()
    a_all = ctx.llm_layers(x_all, sd, len(rows), max(TEXT_LENS), True, 1, True)
    torch.cuda.synchronize()
    yield dict(ctx=ctx, sd=sd, n_seq=len(rows), max_len=max(TEXT_LENS), x0=x0, x_all=x_all, a_all=a_all, spans=spans, mode=mode)
    ctx.close()


def _keep_list(kind, spans):
    rng = np.random.default_rng(5)
    first_text, last = 2 * Q_OPT, R_OPT - 1
    s1, n1 = spans[1]
    must = {first_text, last, s1 + n1 - 2, s1 + n1 - 1}         # ... and both rows of a two-label sequence
    if kind == "one":
        return [417]
    if kind == "all":
        return list(range(R_OPT))
    n = 37 if kind == "37" else 300
    rest = [r for r in rng.permutation(R_OPT).tolist() if r not in must]
    return sorted(must | set(rest[:n - len(must)]))


@pytest.mark.parametrize("kind", ["one", "37", "300", "all"])
def test_kept_rows_equal_all_rows_at_opt_dims(opt_layer, kind):
    o = opt_layer
    keep = _keep_list(kind, o["spans"])
    assert len(keep) == {"one": 1, "37": 37, "300": 300, "all": R_OPT}[kind] and keep == sorted(set(keep))
    x = o["x0"].clone()
    xk, ak = o["ctx"].llm_prefix_rows(x, o["sd"], o["n_seq"], o["max_len"], True, keep, 1)
    kd = torch.tensor(keep, device="cuda")
    assert torch.equal(xk, o["x_all"][kd]), (o["mode"], kind)
    assert torch.equal(ak, o["a_all"][kd]), (o["mode"], kind)
    assert torch.equal(x, o["x0"])                  # one layer: the residual stream before the last layer is the input


def test_bad_keep_lists_are_refused_before_any_launch(opt_layer):
    from devqa_amd import lib
    o = opt_layer
    for bad in ([5, 3, 9], [3, 5, 5, 9], [3, 5, R_OPT], [-1, 4]):
        x = o["x0"].clone()
        with pytest.raises(lib.DevqaError, match=r"\(-1\).*keep_rows"):            # DEVQA_E_ARG
            o["ctx"].llm_prefix_rows(x, o["sd"], o["n_seq"], o["max_len"], True, bad, 1)
        assert torch.equal(x, o["x0"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. grouped post-edit tail
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npad", [8, 272])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_grouped_tail_equals_the_per_edit_loop(mode, npad):
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    adt = torch.bfloat16 if mode == "bf16" else torch.float32
    g = torch.Generator().manual_seed(3)
    seg_rows, Din, N = [12, 1, 40, 33], 640, 320            # N: 2.5 column tiles of 128, 5 of 64
    E, R = len(seg_rows), sum(seg_rows)
    cyc_rows, r = [], 0
    for n in seg_rows:
        cyc_rows.append((r, r + n))
        r += n
    cnt_h = [npad, npad - 3, 1, npad - 3]
    idx_h = torch.empty((E, Din), dtype=torch.int32)
    for e in range(E):
        perm = torch.randperm(Din, generator=g)
        idx_h[e, :cnt_h[e]] = perm[:cnt_h[e]].sort().values.to(torch.int32)
        idx_h[e, cnt_h[e]:] = perm[cnt_h[e]:].to(torch.int32)       # valid but WRONG columns: a kernel that ignores cnt reads them
    idx, cnt = idx_h.cuda(), torch.tensor(cnt_h, dtype=torch.int32).cuda()
    a_tail = torch.randn(R, Din, generator=g).to(adt).cuda()
    delta_op = (torch.randn(E, N, npad, generator=g) * 0.1).to(adt).cuda().contiguous()
    y_pre = torch.randn(R, N, generator=g).cuda()
    # the loop the grouped call replaces (batched.py before it), kept as the reference
    y_ref = y_pre.clone()
    for e, (r0, r1) in enumerate(cyc_rows):
        a_pc = lib.gather_cols(a_tail[r0:r1], idx[e:e + 1], cnt[e:e + 1], npad, per_edit=False)[0]
        lib.gemm(a_pc, delta_op[e], residual=y_ref[r0:r1], out_f32=y_ref[r0:r1])
    assert lib.gemm_grouped_supported(adt, npad)
    seg = lib.TailSegments(cyc_rows, adt, torch.device("cuda:0"))
    y = lib.tail_grouped_(a_tail, seg, idx, cnt, npad, delta_op, y_pre.clone())
    torch.cuda.synchronize()
    assert not torch.equal(y, y_pre)
    assert torch.equal(y, y_ref), (mode, npad, float((y - y_ref).abs().max()))
