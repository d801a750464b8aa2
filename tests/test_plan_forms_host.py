"""Oracle headroom of the plan-form size matrix (tests/plan_forms.py), no GPU: on every entry's weights and batch the fp32
torch-CPU oracle is run against the same oracle in float64.  Its own rel_err / grad_err must stay within a tenth of the 1e-4 the
HIP kernels are held to (tests/test_gpu_plan_forms.py), for every loss and every tensor -- nine tenths of the budget are the
kernels'.  An entry that misses gets another seed or weight scale, never another tolerance."""
import numpy as np
import pytest
import torch

from factorized_amd import engine, synth
from oracle import mfm_oracle as O
from tests import plan_forms as PF
from tests.cases import grad_err, rel_err

TOL = 1e-4


def _run(variant, cs, w, dtype):
    m = O.build(variant, cs["cfgs"])
    O.load_numpy_weights(m, w)
    m.train()
    x, y = torch.from_numpy(cs["x"]), torch.from_numpy(cs["y"])
    if dtype == torch.float64:
        m = m.double()
        x = x.double()
        y = y.double() if y.dtype.is_floating_point else y
    terms = O.loss_terms(m, x, y, cs["cfg"], cs.get("loss_kind", "l1"))
    terms["loss"].backward()
    losses = {k: float(terms[k].detach()) for k in ("disc", "gen", "reg", "loss")}
    grads = {n: (None if p.grad is None else p.grad.numpy().astype(np.float64)) for n, p in m.named_parameters()}
    return losses, grads


def _headroom(variant, cs, seed):
    torch.set_num_threads(4)
    shapes = engine.param_shapes(cs["cfgs"], variant)
    w = synth.make_weights(shapes, seed=seed)
    l32, g32 = _run(variant, cs, w, torch.float32)
    l64, g64 = _run(variant, cs, w, torch.float64)
    for k in l64:
        assert rel_err(l32[k], l64[k]) <= 0.1 * TOL, (k, l32[k], l64[k])
    assert list(g32) == list(g64) == list(shapes)
    for n in g64:
        if g64[n] is None:
            assert g32[n] is None, n
            continue
        assert grad_err(g32[n], g64[n]) <= 0.1 * TOL, (n, grad_err(g32[n], g64[n]))


@pytest.mark.parametrize("name", list(PF.KLEF))
def test_klef_oracle_has_headroom(name):
    _headroom("kl_ef", PF.klef_case(name), PF.WEIGHT_SEED)


@pytest.mark.parametrize("name", list(PF.MFN))
def test_mfn_oracle_has_headroom(name):
    """MFM_KL only: the MFM plans of the same sizes (tests/test_gpu_plan_forms.py) draw their Gaussian sample per run, so the
    fp32 and the float64 oracle would not see the same one"""
    _headroom("kl", PF.mfn_case(name), 1234)          # the weights of test_gpu_mfn_plan._engine
