"""Op-level parity of the T-Patcher patch-neuron kernels (csrc/mend_ops.hip: devqa_tp_neuron_fwd / _bwd and the gated LLaMA-FFN form)
against float64 autograd of the objective they differentiate by hand.  Each kernel is ONE 256-thread workgroup that walks its index
spaces with `t += 256`, `c += 256` and `r += 4` loops; the tiny model configs never take a second trip of any of them, the large shape
here does of all (T > 256, d and d_out > 256, label rows and memory rows > 4), with a repeated label row (two atomic adds into one slot)
and label rows on both sides of index 256.

Bar: max |err| / max |ref| < 2e-5 per output, the bar of the fp32 attention backward (test_attention_bwd_vs_autograd).

Wrong variants of the float64 reference and their distance from the right one at the large shape, as a share of each output's max:
  _act_ref without the ReLU (plain) / with sigmoid for silu (gated)    y 0.08 / 0.06, gk 1.2 / 2.1, gv 0.69 / 2.7
  _memory_loss_ref without the (pm > 0) mask                           losses 0.13 / 0.11, gk 0.020 / 0.022, gb 0.20 / 0.09"""
import pytest
import torch

pytestmark = pytest.mark.gpu

LAMBDA_A, LAMBDA_M, WD = 0.5, 0.3, 0.01


@pytest.fixture(scope="module")
def L():
    import devqa_amd  # noqa: F401
    from devqa_amd import lib
    lib.load()
    return lib


def dev(t):
    return t.to("cuda")


def _act_ref(pre, gated):
    """pre [T, 1] (plain) or [T, 2] (gate, up) -> the new neuron's activation [T]"""
    return torch.nn.functional.silu(pre[:, 0]) * pre[:, 1] if gated else torch.relu(pre[:, 0])


def _memory_loss_ref(pm):
    return torch.exp(pm * (pm > 0)).mean(0).sum()


def _reference(h, hm, K, B, v, ybase, dy, lab, gated):
    """float64: pre [T, nk], y, gradients of sum(y * dy) + lambda_a * loss_a + lambda_m * loss_m + wd / 2 * |params|^2, [loss_a, loss_m]"""
    K, B, v = (t.double().requires_grad_(True) for t in (K, B, v))
    pre = h.double() @ K.T + B
    y = ybase.double() + _act_ref(pre, gated)[lab.long()][:, None] * v
    loss_a = torch.exp(-pre).mean(0).sum()               # summed over the keys, mean over the rows
    loss_m = _memory_loss_ref(hm.double() @ K.T + B)
    obj = (y * dy.double()).sum() + LAMBDA_A * loss_a + LAMBDA_M * loss_m + WD / 2 * ((K * K).sum() + (B * B).sum() + (v * v).sum())
    obj.backward()
    return pre.detach(), y.detach(), K.grad, B.grad, v.grad, torch.stack([loss_a, loss_m]).detach()


def _inputs(T, d, d_out, n_lab, Tm, gated):
    g = torch.Generator().manual_seed(T * 7 + d + int(gated))
    nk = 2 if gated else 1
    h, hm = torch.randn(T, d, generator=g), torch.randn(Tm, d, generator=g)
    K = torch.randn(nk, d, generator=g) / d ** 0.5
    B = 0.1 * torch.randn(nk, generator=g)
    v, dy = 0.1 * torch.randn(d_out, generator=g), 0.1 * torch.randn(n_lab, d_out, generator=g)
    ybase = torch.randn(n_lab, d_out, generator=g)
    lab = [0, 5, 5, 63, 64, 255, 256, T - 2, T - 1] if T > 256 else [1, 4]
    assert len(lab) == n_lab
    # alternate the sign of the (gate) pre-activation along the label rows and the memory rows: both branches of relu / of the mask are taken
    for rows, idx in ((h, sorted(set(lab))), (hm, range(Tm))):
        for i, t in enumerate(idx):
            if (float(rows[t].double() @ K[0].double()) > 0) != (i % 2 == 0):
                rows[t] = -rows[t]
    return h, hm, K, B, v, ybase, dy, torch.tensor(lab, dtype=torch.int32)


def _close(name, got, ref):
    err = (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print("    %-6s max |err| / max |ref| %.3g" % (name, err))
    assert err < 2e-5, (name, err)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("shape", ["tiny", "large"])
def test_tp_neuron_fwd_bwd(L, shape, gated):
    T, d, d_out, n_lab, Tm = (5, 40, 40, 2, 3) if shape == "tiny" else (300, 4096, 4096, 9, 70) if gated else (300, 2560, 2560, 9, 70)
    h, hm, K, B, v, ybase, dy, lab = _inputs(T, d, d_out, n_lab, Tm, gated)
    r_pre, r_y, r_gk, r_gb, r_gv, r_losses = _reference(h, hm, K, B, v, ybase, dy, lab, gated)
    lab_pre = r_pre[lab.long()]
    assert bool((lab_pre[:, 0] > 0).any()) and bool((lab_pre[:, 0] < 0).any())
    pm = hm.double() @ K.double().T + B.double()
    assert bool((pm[:, 0] > 0).any()) and bool((pm[:, 0] < 0).any())
    if gated and shape == "large":                       # ... and of the up key, whose sign the row flips above leave to chance
        assert bool((lab_pre[:, 1] > 0).any()) and bool((lab_pre[:, 1] < 0).any()) and bool((pm[:, 1] > 0).any()) and bool((pm[:, 1] < 0).any())
    print("tp neuron %s gated %d:" % (shape, gated))
    if gated:
        pre, y = L.tp_gated_neuron_fwd(dev(h), dev(K), dev(B), dev(lab), dev(v), dev(ybase))
        assert tuple(pre.shape) == (2, T)
        gk, gb, gv, losses = L.tp_gated_neuron_bwd(dev(h), pre, dev(lab), dev(dy), dev(hm), dev(K), dev(B), dev(v), LAMBDA_A, LAMBDA_M, WD)
        _close("pre", pre, r_pre.T)
    else:
        pre, y = L.tp_neuron_fwd(dev(h), dev(K[0].contiguous()), dev(B), dev(lab), dev(v), dev(ybase))
        gk, gb, gv, losses = L.tp_neuron_bwd(dev(h), pre, dev(lab), dev(dy), dev(hm), dev(K[0].contiguous()), dev(B), dev(v), LAMBDA_A, LAMBDA_M, WD)
        _close("pre", pre, r_pre[:, 0])
        r_gk = r_gk[0]
    torch.cuda.synchronize()
    _close("y", y, r_y)
    _close("gk", gk, r_gk)
    _close("gb", gb, r_gb)
    _close("gv", gv, r_gv)
    _close("losses", losses, r_losses)
