"""losses.WeightedLabelSmoothingCrossEntropy against what the reference's own class gave on the CPU (tests/golden/losses_small.npz,
tools/gen_golden_losses.py): 3 and 10 classes with one, several and all target rows zero.  Loss and logit gradient to 1e-6 relative --
the same op sequence in float32 on the same kind of machine, so a last-bit difference in a reduction's order is all that is allowed."""
import os

import numpy as np
import pytest
import torch

from octcubem_amd import losses

RTOL = 1e-6


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "losses_small.npz"))


def run(z, name):
    x = torch.from_numpy(z[name + "/x"]).clone().requires_grad_(True)
    t = torch.from_numpy(z[name + "/t"])
    loss = losses.WeightedLabelSmoothingCrossEntropy(float(z[name + "/smoothing"]))(x, t)
    loss.backward()
    return x, t, loss.detach(), x.grad


def test_fixture_covers_the_cases(fixture):
    names = [str(n) for n in fixture["cases"]]
    shapes = {(fixture[n + "/x"].shape[1], int((fixture[n + "/t"].sum(-1) == 0).sum()), fixture[n + "/x"].shape[0]) for n in names}
    for C in (3, 10):
        zero = sorted(z for c, z, _ in shapes if c == C)
        rows = {r for c, _, r in shapes if c == C}.pop()
        assert 1 in zero and rows in zero and any(1 < z < rows for z in zero), (C, zero)


@pytest.mark.parametrize("name", ["c3_one", "c3_some", "c10_one", "c10_some", "c10_none"])
def test_loss_and_gradient_match_the_reference(fixture, name):
    x, t, loss, grad = run(fixture, name)
    ref_loss, ref_grad = float(fixture[name + "/loss"]), torch.from_numpy(fixture[name + "/grad"])
    assert loss.dtype == torch.float32 and abs(float(loss) - ref_loss) <= RTOL * abs(ref_loss)
    assert float((grad - ref_grad).norm()) <= RTOL * float(ref_grad.norm())
    assert float((grad - ref_grad).abs().max()) <= RTOL * float(ref_grad.abs().max())
    # rows without a label take no part: their gradient is exactly zero
    assert torch.equal(grad[t.sum(-1) == 0], torch.zeros_like(grad[t.sum(-1) == 0]))


@pytest.mark.parametrize("name", ["c3_all", "c10_all"])
def test_no_valid_row_gives_exactly_zero_and_a_zero_gradient(fixture, name):
    x, t, loss, grad = run(fixture, name)
    assert float(fixture[name + "/loss"]) == 0.0 and not fixture[name + "/grad"].any()
    assert float(loss) == 0.0
    assert grad is not None and torch.equal(grad, torch.zeros_like(grad))


def test_half_logits_are_computed_in_float32_and_autocast_changes_nothing(fixture):
    x = torch.from_numpy(fixture["c10_some/x"])
    t = torch.from_numpy(fixture["c10_some/t"])
    crit = losses.WeightedLabelSmoothingCrossEntropy(0.1)
    want = crit(x.bfloat16().float(), t)
    assert torch.equal(crit(x.bfloat16(), t), want) and want.dtype == torch.float32
    with torch.autocast("cpu", dtype=torch.bfloat16):
        inside = crit(x, t)
    assert inside.dtype == torch.float32 and torch.equal(inside, crit(x, t))
