"""CPU check of tests/fcn_cases.py: the bounds the GPU tests hold the kernel to are met with a wide margin by
torch's own fp32 evaluation of the same restatement at every scale, so they are bounds on the kernel and
not on the reference."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fcn_cases as fc  # noqa: E402

F32 = torch.float32


@pytest.mark.parametrize("S", fc.SCALES)
def test_fp32_restatement_within_bounds(S):
    """fp32 torch against fp64 torch over plain CE and every criterion of loss_cases.CRITERIA: the worst
    figures seen were 3.7e-7 on the loss and 7.6e-6 on dlogits, against the bounds 1e-5 and 2e-4."""
    torch.set_num_threads(max(1, min(8, torch.get_num_threads())))
    worst_l = worst_g = 0.0
    for shape in fc.CPU_SHAPES:
        lg, lab = fc.make_inputs(shape, S)
        for name in fc.NAMES:
            ref = fc.reference_of(fc.criterion_of(name, shape[3]), lg, lab, S)
            got = fc.reference_of(fc.criterion_of(name, shape[3]), lg, lab, S, dtype=F32)
            le = abs(got.loss.item() - ref.loss.item()) / abs(ref.loss.item())
            ge = fc.relerr(got.dlogits, ref.dlogits)
            worst_l, worst_g = max(worst_l, le), max(worst_g, ge)
            assert le < fc.LOSS_TOL[F32], (S, shape, name, le)
            assert ge < 2 * fc.TOL[F32], (S, shape, name, ge)
    print(f"x{S}: worst fp32 loss rel err {worst_l:.2e}, dlogits rel err {worst_g:.2e}")


def test_inputs_scale_with_S():
    """The ignored rectangle scales with S, labels are (B, S h, S w), and a map larger than 1.25 x 1.75 cells
    has both valid and ignored pixels."""
    for S in fc.SCALES:
        lg, lab = fc.make_inputs((2, 4, 5, 40), S)
        assert lab.shape == (2, 4 * S, 5 * S) and lg.shape == (2, 4, 5, 40)
        ign = lab == fc.IGNORE
        assert ign.any() and (~ign).any()
        f = S // 4
        assert ign[:, 5 * f:30 * f, 7 * f:40 * f].all() and not ign[:, :5 * f].any()
        _, lab = fc.make_inputs((1, 1, 1, 5), S, ignored="all")
        assert (lab == fc.IGNORE).all()
