"""Launch sequences of the recurrence launchers (lstm_seq.hip: seq_launch's forms; lstm_seq_small.hip): for batch sizes on either
side of every routing threshold the code names, and for each switch that takes a form away, two training steps of the canonical
MFM_KL_EF engine must issue the launches recorded in tests/golden/seq_launch_table.json -- per slot of the plan's timing table --
and leave the role-workgroup forms on or off as recorded.

The table was recorded from the commit BEFORE the launchers were rewritten around an explicit launch form (run this file as a
program on that commit: `python -m tests.test_gpu_seq_forms OUT.json`), never from the code under test.  It is a function of the
CU count (every threshold is a multiple of it), which is stored with it: another device skips.

What the table can and cannot see: a slot counts the launches of one REGION of the step, so a form that falls back to separate
launches shows up (proj_gemm, dw_gemm, latent_fwd / latent_bwd, the tails' own launch), and so does a recurrence split into
several launches (MFMA path: encoders and decoders; step-by-step path).  Forms that replace one launch by one launch of the same
region are charged to the same slot: the image-only forms (writer blocks, wt_img / wf_img operands) count as the plain launch,
and the decoder launch with tail / head blocks as the decoder launch -- those are told apart only through the slots of the
launches they make unnecessary and through the two role options."""
import json
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
T = 3
STEPS = 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_launch_table.json")

# (id, B, precision, switches set for the case)
CASES = [
    ("b1", 1, "fp32", {}),
    ("b32", 32, "fp32", {}),                                   # projection roles stop at 32 rows
    ("b33", 33, "fp32", {}),
    ("b48", 48, "fp32", {}),                                   # weight-gradient roles: only with MFM_DW_FOLD_MAXITER
    ("b48_maxiter", 48, "fp32", {"MFM_DW_FOLD_MAXITER": "99"}),
    ("b96", 96, "fp32", {}),                                   # count * B > CUs: sorted descriptors, no images
    ("b512", 512, "fp32", {}),                                 # four-row tiles
    ("b640", 640, "fp32", {}),                                 # MFMA path
    ("bf16_b32", 32, "bf16", {}),                              # either side of MFM_BF16_SEQ_MINB
    ("bf16_b160", 160, "bf16", {}),
    ("b32_rows4", 32, "fp32", {"MFM_SEQ_ROWS": "4"}),
    ("b32_stepwise", 32, "fp32", {"MFM_SEQ_STEPWISE": "1"}),
    ("b32_no_tail", 32, "fp32", {"MFM_LATENT_TAIL": "0"}),
    ("b32_no_bwd_head", 32, "fp32", {"MFM_LATENT_BWD_HEAD": "0"}),
    ("b32_no_wt_img", 32, "fp32", {"MFM_WT_IMG": "0"}),
]
SWITCHES = sorted({k for c in CASES for k in c[3]})


def _cus():
    from factorized_amd import _lib
    return int(_lib.lib().mfm_device_cus())


def _observe(B, precision):
    """Two training steps with every timer on: launches per slot, the role options, status word and loss."""
    import torch
    from factorized_amd import _lib, configs, engine, synth
    cfgs = configs.canonical_configs(dropout=False)
    e = engine.MFMEngine(cfgs, precision=precision)
    e.load_weights(synth.make_weights(e.layout.shapes, seed=1234))
    xn, yn = synth.make_batch(cfgs[0]["input_dims"], B, T, seed=7)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    e.set_timing(T, B, (1 << 30) - 1)
    for _ in range(STEPS):
        losses = e.train_step(x, y)
    torch.cuda.synchronize()
    tab = e.collect_timing(T, B)
    e.set_timing(T, B, 0)
    seen = {"launches": {k: int(v["count"]) for k, v in sorted(tab.items()) if v["count"]}}
    p = e.plan(T, B)
    for opt in ("proj_roles_active", "dw_roles_active"):
        try:
            seen[opt] = p.get_option(opt)
        except _lib.MfmError:
            seen[opt] = None          # (not exposed by this plan)
    return seen, e.check_status(), e.loss_dict(losses)["loss"]


def _set_switches(setenv, delenv, switches):
    for k in SWITCHES:
        if k in switches:
            setenv(k, switches[k])
        else:
            delenv(k)


@pytest.fixture(scope="module")
def table():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(GOLDEN) as f:
        tab = json.load(f)
    if tab["cus"] != _cus():
        pytest.skip("launch table recorded for %d CUs, this device has %d" % (tab["cus"], _cus()))
    assert tab["T"] == T and tab["steps"] == STEPS
    return tab["cases"]


@pytest.mark.parametrize("name,B,precision,switches", CASES, ids=[c[0] for c in CASES])
def test_launch_sequence_as_recorded(table, name, B, precision, switches, monkeypatch):
    _set_switches(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), switches)
    seen, status, loss = _observe(B, precision)
    print(name, json.dumps(seen, sort_keys=True), "status", status, "loss", loss)
    assert status == 0
    assert math.isfinite(loss)
    assert seen == table[name], (seen, table[name])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {"cus": _cus(), "T": T, "steps": STEPS, "cases": {}}
    for name, B, precision, switches in CASES:
        _set_switches(os.environ.__setitem__, lambda k: os.environ.pop(k, None), switches)
        seen, status, loss = _observe(B, precision)
        assert status == 0 and math.isfinite(loss), (name, status, loss)
        out["cases"][name] = seen
        print(name, json.dumps(seen, sort_keys=True), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
