"""tests/_vgg_bf16_emulation.py against the fp64 oracle, on the CPU: with the roundings off the emulation IS
oracle.models.vgg19_block5_conv4 (forward exactly, image gradient to fp64 rounding); with them on, the feature distance d_ref and the
gradient-rounding chain error e_chain -- the two figures the GPU tests' bounds are multiples of -- stay under their caps.  The figures are
printed (pytest -s) and appended to the parity report."""
import pytest
import torch

import _vgg_bf16_emulation as V
from conftest import report
from oracle import models as M


def _say(line):
    print(line)
    report(line)


@pytest.mark.parametrize("shape", V.SHAPES)
def test_roundings_off_is_the_oracle(shape):
    ref = V.reference(shape)
    w = ref["w"]
    xt = torch.tensor(ref["x"], dtype=torch.float64, requires_grad=True)
    taps = []
    f = V.forward(w, xt, False, taps)
    assert torch.equal(f.detach(), ref["f_oracle"])
    assert all(torch.equal(a.detach(), b) for a, b in zip(taps, ref["taps_oracle"]))
    # image gradient of the MSE feature loss against shifted features: autograd of the oracle's own function against the linear backward
    target = torch.roll(ref["f_oracle"], 1, 0) if shape[0] > 1 else ref["f_oracle"] * 0.5
    fo = M.vgg19_block5_conv4(w, xt)
    (g_or,) = torch.autograd.grad(((fo - target) ** 2).mean(), xt)
    dz = V.loss_grad(target, ref["f_oracle"], "mse", 1.0, round_grads=False).permute(0, 3, 1, 2)
    g_em = V.backward(w, ref["taps_oracle"], dz, (shape[0], 3, shape[1], shape[2]), bf16_kernels=False, round_grads=False)
    err = V.rel_l2(g_em.permute(0, 2, 3, 1), g_or)
    _say("vgg bf16 emulation %s roundings off: image gradient rel L2 against autograd %.2e" % (shape, err))
    assert err < 1e-12


@pytest.mark.parametrize("shape", V.SHAPES)
def test_feature_distance_and_chain_error_under_their_caps(shape):
    ref = V.reference(shape)
    flips = max(float(((a > 0) != (b > 0)).double().mean()) for a, b in zip(ref["taps_emu"], ref["taps_oracle"]))
    e_chain = V.chain_error(shape)
    _say("vgg bf16 emulation %s: d_ref=%.2e  worst layer's flipped ReLU masks=%.2e  e_chain=%.2e" % (shape, ref["d_ref"], flips, e_chain))
    assert 0 < ref["d_ref"] < V.D_REF_CAP
    assert 0 < e_chain < V.E_CHAIN_CAP


def test_loss_gradient_helper_matches_autograd():
    g = torch.Generator().manual_seed(2)
    t, p = V.r_bf16(torch.randn(3, 5, 7, generator=g, dtype=torch.float64)), torch.randn(3, 5, 7, generator=g, dtype=torch.float64)
    for kind in ("mse", "mae"):
        z = p.clone().requires_grad_(True)
        a = torch.relu(z)
        loss = ((a - t) ** 2).mean() if kind == "mse" else (a - t).abs().mean()
        (gz,) = torch.autograd.grad(3.0 * loss, z)
        assert torch.allclose(V.loss_grad(t, torch.relu(p), kind, 3.0, round_grads=False), gz, rtol=1e-14, atol=0)
        assert abs(V.loss_value(t, torch.relu(p), kind) - float(loss.detach())) < 1e-15
