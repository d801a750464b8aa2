"""What tests/test_gpu_dropout.py asserts about ONE training-mode call of the fused plan, as a function: the kernel form the
call is there for, the dropout masks the kernels drew (read back from the plan's latent record), and -- with those masks
injected into the CPU oracle -- forward losses, every gradient and, for train_step, the parameters after one Adam step.

The masks come from a counter-based generator (common.h rng_uniform), a pure function of (seed, call number, op index, row,
column) that every latent kernel form restates at its own draw site; the backward forms read the stored masks at sites of
their own.  A site that scaled differently, dropped the row term of the stream index or read another site's mask segment
would still train, just wrongly: what catches it here is that the ORACLE's gradients under the masks that were read back
must equal the kernels' at 1e-4."""
import numpy as np
import torch

from oracle import mfm_oracle as O
from tests import cases

TOL = 1e-4
SITES = {"zl_to_fl": ("zl_to_fl_dropout", "l"), "za_to_fa": ("za_to_fa_dropout", "a"),
         "zv_to_fv": ("zv_to_fv_dropout", "v"), "zy_to_fy": ("zy_to_fy_dropout", "y"),
         "fy_to_y": ("fy_to_y_dropout", None)}
P = dict(zl_to_fl_dropout=0.2, za_to_fa_dropout=0.5, zv_to_fv_dropout=0.7, zy_to_fy_dropout=0.3, fy_to_y_dropout=0.4)
ENTRIES = ("forward", "grad_step", "train_step")
STATS_FROM = 1000          # mask elements (B x width) from which a site's kept fraction is held to 5 sigma of the binomial


class _FixedMask(torch.nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask


def _seg(a, lay, kind, site):
    return a[:, lay[kind][site]: lay[kind][site] + lay["width"][site]]


def read_masks(e, T, B):
    rec, _, lay = e.latent_record(T, B)
    rec = rec.cpu().numpy()
    return {site: _seg(rec, lay, "mask", site).copy() for site in SITES}


def _run(e, entry, x, y):
    """one training-mode call through `entry`; the device tensor of its loss slots"""
    if entry == "forward":
        return e.forward(x, y, train=True, want_xhat=False)["losses"]
    if entry == "grad_step":
        return e.grad_step(x, y)
    assert entry == "train_step", entry
    return e.train_step(x, y)


def launches(e, T, B):
    """launches per slot of the plan's timing table since set_timing (as tests/test_gpu_seq_forms._observe reads it)"""
    torch.cuda.synchronize()
    return {k: int(v["count"]) for k, v in sorted(e.collect_timing(T, B).items()) if v["count"]}


def check_dropout(key, e, w, cfgs, xn, yn, entry="forward", form=None, own_launch=None, slots=None, loss_kind="l1",
                  stats_from=STATS_FROM):
    """`e`: a FRESH engine holding the weights `w` (its first call is made here, so that the masks of two engines can be compared
    call for call).  `form`: fields of MFMEngine.latent_form() that must hold exactly.  `own_launch`: True / False -- the timing
    table of the checked call must (not) show a latent_fwd and a latent_bwd launch (False: the chains ran inside the recurrence
    launches); `slots`: further slots of that table with the count they must show.  Returns dict(masks, next_masks, worst)."""
    assert entry in ENTRIES, entry
    cfg = cfgs[0]
    T, B = xn.shape[0], xn.shape[1]
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    # ---- the form, before any number: a case that ran another form than the one it is there for fails here
    got_form = e.latent_form(T, B)
    print(key, entry, "form", got_form)
    for k, v in (form or {}).items():
        assert got_form[k] == v, (k, got_form[k], v, got_form)
    e.set_timing(T, B, (1 << 30) - 1)
    losses = _run(e, entry, x, y)
    rec, grd, lay = e.latent_record(T, B)
    assert lay["row_path"] == got_form["row_path"]
    rec = rec.cpu().numpy().copy()
    ld = e.loss_dict(losses)
    masks = {}
    for site, (pkey, seg) in SITES.items():
        p = cfg[pkey]
        n = lay["width"][site]
        mk = _seg(rec, lay, "mask", site)
        assert mk.shape == (B, n)
        if p == 0.0:
            assert np.all(mk == 1.0), site                                  # no dropout at this site: exactly 1.0 everywhere
        else:
            # the plan holds p as a float32 (MfmPlanConfig): 1 / (1 - p) of THAT number
            keep = 1.0 / (1.0 - float(np.float32(p)))
            assert np.all((mk == 0.0) | (np.abs(mk - keep) < 1e-6)), site          # 0 or 1/(1-p), nothing else
            frac = float((mk != 0.0).mean())
            if mk.size >= stats_from:
                sigma = np.sqrt(p * (1 - p) / mk.size)
                assert abs(frac - (1 - p)) < 5 * sigma + 1e-9, (site, frac, 1 - p)
            # rows draw different masks (the generator is keyed by row and column, not by column alone)
            if B > 1:
                assert not np.all(mk == mk[:1]), site
        # the stored activation is relu(fc1(input)) * mask
        if seg is None:
            inp = rec[:, lay["f"]["y"]: lay["f"]["y"] + lay["width"]["zy_to_fy"]]
            wt, bs = w["fy_to_y_fc1.weight"], w["fy_to_y_fc1.bias"]
        else:
            inp = rec[:, lay["mu"][seg]: lay["mu"][seg] + lay["z_n"][seg]]
            wt, bs = w[site + "_fc1.weight"], w[site + "_fc1.bias"]
        want = np.maximum(inp.astype(np.float64) @ wt.T.astype(np.float64) + bs, 0.0) * mk
        got = _seg(rec, lay, "act", site)
        assert np.max(np.abs(got - want)) < 1e-5 * max(1.0, np.abs(want).max()), site
        masks[site] = mk.copy()
    if entry == "forward":
        e.backward(x, y, stage=0)
    seen = launches(e, T, B)
    e.set_timing(T, B, 0)
    print(key, entry, "launches", seen)
    if own_launch is not None:
        for k in ("latent_fwd", "latent_bwd"):
            assert (seen.get(k, 0) > 0) == own_launch, (k, own_launch, seen)
    for k, v in (slots or {}).items():
        assert seen.get(k, 0) == v, (k, v, seen)
    assert e.check_status() == 0
    # ---- the same masks in the oracle: losses and every gradient must agree
    m = O.build("kl_ef", cfgs)
    O.load_numpy_weights(m, w)
    m.train()
    for site, (pkey, _) in SITES.items():
        setattr(m, pkey, _FixedMask(torch.from_numpy(masks[site])))
    torch.set_num_threads(4)
    terms = O.loss_terms(m, torch.from_numpy(xn), torch.from_numpy(yn), cfg, loss_kind)
    terms["loss"].backward()
    for k in ("disc", "gen", "reg", "loss"):
        ref = float(terms[k].detach())
        assert abs(ld[k] - ref) <= TOL * max(abs(ref), 1e-3), (k, ld[k], ref)
    gv = e.grad_views()
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        err = cases.grad_err(gv[n].cpu().numpy(), p.grad.numpy())
        if err > worst[1]:
            worst = (n, err)
    print("%s %s worst gradient: %s %.3e" % (key, entry, worst[0], worst[1]))
    cases.report("dropout_grad_%s_%s" % (key, entry), worst[1])
    assert worst[1] < TOL, "worst gradient mismatch %s: %.3e" % worst
    # dropped units carry exactly no gradient into their pre-activation
    g = grd.cpu().numpy()
    for site in SITES:
        seg = _seg(g, lay, "act", site)
        assert np.all(seg[masks[site] == 0.0] == 0.0), site
        # (not vacuously: some unit of the site was kept with its relu open -- a single row of a narrow site may have none)
        live = (masks[site] != 0.0) & (_seg(rec, lay, "act", site) > 0.0)
        assert live.any() or B * lay["width"][site] < 64, site
        assert np.any(seg != 0.0) == bool(live.any()), site
    if entry == "train_step":
        # one Adam step under the same masks: the per-tensor rule of tests/test_gpu_mfn_plan.py (2e-5 on the elements whose
        # gradient is not noise, and nowhere further apart than the lr a step can move a parameter), for ONE step
        g0 = {n: p.grad.detach().clone().numpy() for n, p in m.named_parameters()}
        torch.optim.Adam(m.parameters()).step()
        pv = e.param_views()
        for n, p in m.named_parameters():
            d = np.abs(pv[n].cpu().numpy() - p.detach().numpy())
            sig = np.abs(g0[n]) > 1e-3 * np.abs(g0[n]).max()
            if sig.any():
                assert d[sig].max() < 2e-5, (n, d[sig].max())
            assert d.max() < 1.01 * 1e-3, n
    # ---- fresh masks on the next call through the same entry; eval mode applies none
    _run(e, entry, x, y)
    nxt = read_masks(e, T, B)
    for site, (pkey, _) in SITES.items():
        if cfg[pkey] == 0.0:
            assert np.all(nxt[site] == 1.0), site
        else:
            assert not np.array_equal(nxt[site], masks[site]), site
    e.forward(x, y, train=False, want_xhat=False)
    for site, a in read_masks(e, T, B).items():
        assert np.all(a == 1.0), site
    assert e.check_status() == 0
    return dict(masks=masks, next_masks=nxt, worst=worst[1], form=got_form, launches=seen)
