"""The fairness term of the loss without a GPU: ffm_ce_fair_loss is declared, bound and exported beside the unchanged
ffm_ce_loss (ABI still 14), it validates its arguments before any launch, the command line carries --lambda_fairness /
--fairness_grad into the config, and the closed form the kernel implements (include/ffm_hip.h) is the autograd gradient of
CE + lambda * F with the term not detached."""
import ctypes
import os
import re

import pytest
import torch

from fairfedmed_amd import _lib
from tests import fairness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ffm_ce_fair_loss"


def test_entry_point_is_declared_bound_and_exported():
    from fairfedmed_amd import build as B
    protos = {n: (rt, params) for rt, n, params in B.api_prototypes()}
    assert NAME in protos and NAME in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    rt, params = protos[NAME]
    assert rt == "int" and [a for _, a in params] == [
        "logits_img", "label", "attr", "logits", "prob", "loss", "terms", "gstat", "dlogits_img", "finite_flag",
        "nb", "S", "n_cls", "G", "lambda", "with_grad", "stream"]
    assert [t for t, _ in params] == ["const float*", "const int64_t*", "const int32_t*"] + ["float*"] * 6 + ["int32_t*"] \
        + ["int"] * 4 + ["float", "int", "void*"]
    sig = _lib.SIGNATURES[NAME]
    assert len(sig) == len(params) and sig[14] is ctypes.c_float and all(s is ctypes.c_int32 for s in sig[10:14] + [sig[15]])
    # ffm_ce_loss keeps its prototype, and the header cites the reference lines and states the formulas
    assert [a for _, a in protos["ffm_ce_loss"][1]] == ["logits_img", "label", "logits", "prob", "loss", "dlogits_img",
                                                       "finite_flag", "nb", "S", "n_cls", "stream"]
    raw = open(B.HEADER).read()
    doc = raw[raw.index("ffm_ce_loss plus the group-confidence-gap term"):raw.index(f"int {NAME}(")]
    for needle in ("trainers/GLP_OT_SVLoRA.py:908", "kappa_g", "extension beyond the reference", "fixed-order"):
        assert needle in doc, needle
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"`{NAME}`" in md


def test_abi_version_is_still_14():
    assert _lib.ABI_VERSION == 14 and _lib.load().ffm_abi_version() == 14
    hdr = open(os.path.join(ROOT, "include", "ffm_hip.h")).read()
    assert re.search(r"#define FFM_ABI_VERSION 14\b", hdr)


def test_invalid_arguments_return_einval_before_any_launch():
    """Null pointers (gstat and finite_flag may be NULL), nb / S / n_cls <= 0, n_cls > 8, G <= 0 and G > FFM_MAX_GROUPS:
    -1 with no GPU in sight (the pointers are only compared with NULL)."""
    f = getattr(_lib.load(), NAME)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    good = [p] * 10 + [8, 1, 2, 3, 0.5, 1, None]
    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        a = list(good)
        a[i] = None
        assert f(*a) == -1, ("null argument", i)
    for idx, bad in ((10, 0), (10, -3), (11, 0), (11, -1), (12, 0), (12, 9), (13, 0), (13, -1), (13, 9)):
        a = list(good)
        a[idx] = bad
        # (gstat / finite_flag NULL as well: a bad size must be refused before anything could run)
        a[7] = a[9] = None
        assert f(*a) == -1, (idx, bad)


def test_command_line_carries_the_two_flags():
    from fairfedmed_amd import federated_main as FM
    base = ["--root", "DATA/", "--trainer", "GLP_OT_SVLoRA"]
    t = FM.setup_cfg(FM.build_parser().parse_args(base)).TRAINER
    assert (t.LAMBDA_FAIRNESS, t.FAIRNESS_GRAD) == (0.0, False)
    t = FM.setup_cfg(FM.build_parser().parse_args(base + ["--lambda_fairness", "0.5"])).TRAINER
    assert (t.LAMBDA_FAIRNESS, t.FAIRNESS_GRAD) == (0.5, False)          # the reference's detached term stays the default
    t = FM.setup_cfg(FM.build_parser().parse_args(base + ["--lambda_fairness", "0.25", "--fairness_grad"])).TRAINER
    assert (t.LAMBDA_FAIRNESS, t.FAIRNESS_GRAD) == (0.25, True)


@pytest.mark.parametrize("case", R.all_kernel_inputs(), ids=lambda c: c[0])
def test_closed_form_is_the_autograd_gradient_of_the_undetached_term(case):
    """float64: the header's kappa formula against autograd through torch.stack'ed group means, on every input the GPU
    test feeds the kernel; the same formulas in fp32 stay within the GPU test's bounds with two orders of margin."""
    _, logits_img, y, a, G, S = case
    z = R.slice_mean(logits_img, len(y), S)
    assert R.min_gap(z, y, a, G) >= R.MIN_GAP
    loss, cls, F, dz = R.autograd_ref(z, y, a, G, R.LAMBDA)
    l2, c2, F2, dz2, gstat = R.closed_form(z, y, a, G, R.LAMBDA)
    assert float(F) > 0 and abs(float(l2 - loss)) <= 1e-14 and abs(float(c2 - cls)) <= 1e-14 and abs(float(F2 - F)) <= 1e-15
    assert float((dz2 - dz).abs().max()) <= 1e-15
    assert not torch.equal(dz2, R.closed_form(z, y, a, G, R.LAMBDA, with_grad=False)[3])
    present, m, _, _ = R.group_stats(z, y, a, G)
    assert [g for g in range(G) if gstat[g, 1] > 0] == present and float((gstat[present, 0] - m).abs().max()) <= 1e-15
    l32, _, F32, dz32, _ = R.closed_form(z.float(), y, a, G, R.LAMBDA, dtype=torch.float32)
    assert abs(float(F32) - float(F)) <= 2e-6 * float(F) and abs(float(l32) - float(loss)) <= 2e-6 * float(loss)
    assert float((dz32.double() - dz).abs().max()) <= 2e-7 * float(dz.abs().max())


def test_closed_form_edge_rules():
    """One present group, and every attribute outside [0, G): F = 0 and the gradient is the cross-entropy's alone; a sample
    outside the groups keeps its cross-entropy gradient and takes no part in the statistics."""
    z, y, a = R.draw(8, 2, 3, 11)
    for attr in (torch.full((8,), 2), torch.full((8,), -1), torch.full((8,), 3)):
        loss, cls, F, dz, gstat = R.closed_form(z, y, attr, 3, R.LAMBDA)
        assert float(F) == 0.0 and float(loss) == float(cls)
        assert torch.equal(dz, R.closed_form(z, y, attr, 3, R.LAMBDA, with_grad=False)[3])
        assert float((R.autograd_ref(z, y, attr, 3, R.LAMBDA)[3] - dz).abs().max()) <= 1e-15
    out = a.clone()
    out[0] = -1
    _, _, F, dz, gstat = R.closed_form(z, y, out, 3, R.LAMBDA)
    ce = R.closed_form(z, y, out, 3, R.LAMBDA, with_grad=False)[3]
    assert torch.equal(dz[0], ce[0]) and not torch.equal(dz[1:], ce[1:]) and int(gstat[:, 1].sum()) == 7
    assert float((R.autograd_ref(z, y, out, 3, R.LAMBDA)[3] - dz).abs().max()) <= 1e-15
