"""The refusal rule of the engine's no-plan entries (factorized_amd/_infer.py, InferMixin._run_fused) on the MI355X: an entry that
answers MFM_ERR_UNSUPPORTED at sizes within the on-chip recurrence (no hidden size above 128: the LDS kind of refusal, which
depends on the shape) is NOT remembered and stores nothing -- predict, objective and predict_zeros return the fallback's result,
encode and decode raise and the model composes -- and the next call reaches the real entry again.  The refusal is the library
function wrapped to answer MFM_ERR_UNSUPPORTED a given number of times, on the smallest golden case (B = 33, T = 7: a ragged last
four-row tile).  Numeric bound: the project's 1e-4 relative fp32 tolerance (tests.cases.rel_err; scalars with the 1e-3 floor
of test_gpu_objective.py)."""
import pytest
import torch

from factorized_amd import _lib, synth
from tests import cases
from tests.cases import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
CASE = "klef_b33_t7"


def _model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from factorized_amd import mfm_model as M
    cs = cases.load_case(CASE)
    model = M.MFM_KL_EF(*cs["cfgs"])
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    w = synth.make_weights(shapes, seed=1234)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    return model.to("cuda"), cs


def _host(ts):
    """copies on the host (the engine reuses its result tensors)"""
    return [None if t is None else t.detach().cpu().numpy().copy() for t in ts]


_TRUTH = {}


def _truth():
    """the un-patched results of the five entries, computed once and left unchanged"""
    if not _TRUTH:
        model, cs = _model()
        e = model.engine
        x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
        p = e.predict(x, y)
        enc = e.encode(x)
        _TRUTH.update(predict=_host([p["y_hat"], p["loss"]]), objective=_host(e.objective(x, y)), zeros=_host(e.predict_zeros(x, y)),
                      encode=_host(enc), decode=_host(e.decode(*enc[:4], cs["T"])))
        assert not e._plans          # (every one of them came from its fused entry)
    return _TRUTH


def _refusing(monkeypatch, entry, times=1):
    """the library function `entry` answers MFM_ERR_UNSUPPORTED `times` times and is itself again afterwards; -> the call log"""
    L, log = _lib.lib(), []
    real = getattr(L, entry)

    def fn(*a):
        log.append(entry)
        return _lib.MFM_ERR_UNSUPPORTED if len(log) <= times else real(*a)
    monkeypatch.setattr(L, entry, fn, raising=True)
    return log


def _close(tag, got, want):
    """every tensor within TOL of the un-patched one (losses, 0-d or [3]: each element on its own, with the floor); prints each
    figure before it asserts"""
    assert len(got) == len(want)
    errs = []
    for g, w in zip(_host(got), want):
        assert g.shape == w.shape
        if w.ndim < 2:
            errs += [abs(float(a) - float(b)) / max(abs(float(b)), 1e-3) for a, b in zip(g.reshape(-1), w.reshape(-1))]
        else:
            errs.append(rel_err(g, w))
    print("%s %s" % (tag, " ".join("%.2e" % e for e in errs)))
    assert max(errs) <= TOL, (tag, errs)


def _same(got, want):
    return all((g == w).all() for g, w in zip(_host(got), want))


FALLBACK = {
    "predict": ("mfm_predict_klef", lambda e, x, y: (lambda p: [p["y_hat"], p["loss"]])(e.predict(x, y))),
    "objective": ("mfm_objective_klef", lambda e, x, y: list(e.objective(x, y))),
    "zeros": ("mfm_predict_zeros_klef", lambda e, x, y: list(e.predict_zeros(x, y))),
}


@pytest.mark.parametrize("name", sorted(FALLBACK))
def test_a_refusal_at_resident_sizes_falls_back_and_is_not_remembered(name, monkeypatch):
    entry, run = FALLBACK[name]
    want = _truth()[name]
    model, cs = _model()
    e = model.engine
    x, y = torch.from_numpy(cs["x"]).cuda(), torch.from_numpy(cs["y"]).cuda()
    log = _refusing(monkeypatch, entry)
    got = run(e, x, y)
    assert log == [entry] and len(e._plans) == 1                     # the entry was asked, the plan's forward answered
    _close("refused_once " + name, got, want)
    assert getattr(e, "_%s_refused" % name) is False                 # (no hidden size is above 128)
    assert not e.__dict__.get("_%s_bufs" % name)                     # nothing was stored for the refused call
    again = run(e, x, y)
    assert log == [entry] * 2 and len(e.__dict__["_%s_bufs" % name]) == 1          # the real entry, reached again
    assert _same(again, want)                                        # ... and its bits


def test_encode_and_decode_raise_compose_and_are_not_remembered(monkeypatch):
    want = _truth()
    model, cs = _model()
    e = model.engine
    x, T = torch.from_numpy(cs["x"]).cuda(), cs["T"]
    z = [torch.from_numpy(f).cuda() for f in want["encode"][:4]]
    enc_log = _refusing(monkeypatch, "mfm_encode_klef", times=2)
    dec_log = _refusing(monkeypatch, "mfm_decode_factors", times=2)
    with pytest.raises(_lib.MfmUnsupported):
        e.encode(x)
    with pytest.raises(_lib.MfmUnsupported):
        e.decode(*z, T)
    assert e._encode_refused is False and e._decode_refused is False
    _close("refused encode", list(model.encode(x)), want["encode"])              # (the second refusal: the model composes)
    _close("refused decode", model.decode(*z, T), want["decode"])
    assert len(enc_log) == 2 and len(dec_log) == 2
    assert e._encode_refused is False and e._decode_refused is False
    assert not e.__dict__.get("_encode_bufs") and not e.__dict__.get("_decode_bufs")
    assert _same(model.encode(x), want["encode"]) and _same(model.decode(*z, T), want["decode"])      # the real entries again
    assert len(enc_log) == 3 and len(dec_log) == 3 and len(e._encode_bufs) == 1 and len(e._decode_bufs) == 1
