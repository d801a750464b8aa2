"""ms per step of the reference's UNCHANGED loop (mfm_mosi.py:427-441 incl. its per-step .item()) on MFM_KL_EF, B=32, T=20:
stock torch.optim.Adam vs factorized_amd.optim.Adam, per-tensor autograd path vs flat gradients, torch.optim.SGD vs
factorized_amd.optim.SGD (lr 0.01, momentum 0.9), torch.optim.AdamW vs factorized_amd.optim.AdamW (and AMSGrad, two parameter
groups), and the fused engine call."""
import os, time
import torch, torch.nn as nn
from _bench_common import B, T, cfgs, config, d_a, d_l, loop, mosi_batch, need_gpu, timed, timed_steps
from factorized_amd.mfm_model import MFM_KL_EF
import factorized_amd.optim as optim

need_gpu("bench_dropin.py")
X, y = mosi_batch()
for name, opt_cls, fast, item in (("torch.optim.Adam, per-tensor autograd (round 2)", torch.optim.Adam, False, True),
                                  ("torch.optim.Adam, flat gradients", torch.optim.Adam, True, True),
                                  ("factorized_amd.optim.Adam, flat gradients", optim.Adam, True, True),
                                  ("factorized_amd.optim.Adam, flat gradients, no per-step .item()", optim.Adam, True, False)):
    # (the per-tensor runs leave cyclic garbage holding device tensors behind: measured, the next configuration's per-step
    # `.item()` then costs 0.2-0.3 ms more -- a property of this script's history, not of the path)
    import gc
    model = optimizer = None
    gc.collect(); torch.cuda.empty_cache()
    model = MFM_KL_EF(*cfgs)
    model.fast_grads = fast
    optimizer = opt_cls(model.parameters())
    model = model.to("cuda")
    model.train()
    print("%-70s %.3f ms/step" % (name, timed_steps(lambda k: loop(model, optimizer, k, item), 300, 30)))
# the reference's other optimizer line (mfm_mosi.py:404) at the canonical lr 0.01, momentum 0.9, flat gradients
for name, opt_cls, item in (("torch.optim.SGD(lr=0.01, momentum=0.9), flat gradients", torch.optim.SGD, True),
                            ("factorized_amd.optim.SGD(lr=0.01, momentum=0.9), flat gradients", optim.SGD, True),
                            ("factorized_amd.optim.SGD(lr=0.01, momentum=0.9), no per-step .item()", optim.SGD, False)):
    import gc
    model = optimizer = None
    gc.collect(); torch.cuda.empty_cache()
    model = MFM_KL_EF(*cfgs)
    optimizer = opt_cls(model.parameters(), lr=config["lr"], momentum=config["momentum"])
    model = model.to("cuda")
    model.train()
    print("%-70s %.3f ms/step" % (name, timed_steps(lambda k: loop(model, optimizer, k, item), 300, 30)))
# torch.optim.Adam's other options (span kernel mfm_adam_ext_flat_spans_guarded): AdamW with weight_decay 1e-2, AMSGrad, two
# parameter groups; the plain Adam line repeated in between shows the spread of this run
def two_groups(m):
    enc = ("encoder_l.", "encoder_a.", "encoder_v.", "ef_encoder.")
    return [{"params": [p for n, p in m.named_parameters() if n.startswith(enc)], "lr": 1e-4},
            {"params": [p for n, p in m.named_parameters() if not n.startswith(enc)]}]


for name, make, item in (("torch.optim.AdamW(weight_decay=1e-2), flat gradients", lambda m: torch.optim.AdamW(m.parameters(), weight_decay=1e-2), True),
                         ("factorized_amd.optim.AdamW(weight_decay=1e-2), flat gradients", lambda m: optim.AdamW(m.parameters(), weight_decay=1e-2), True),
                         ("factorized_amd.optim.Adam, flat gradients (again)", lambda m: optim.Adam(m.parameters()), True),
                         ("factorized_amd.optim.AdamW(weight_decay=1e-2), no per-step .item()", lambda m: optim.AdamW(m.parameters(), weight_decay=1e-2), False),
                         ("factorized_amd.optim.Adam, no per-step .item() (again)", lambda m: optim.Adam(m.parameters()), False),
                         ("factorized_amd.optim.Adam(weight_decay=1e-4, amsgrad=True), flat gradients", lambda m: optim.Adam(m.parameters(), weight_decay=1e-4, amsgrad=True), True),
                         ("factorized_amd.optim.AdamW, encoders in their own group", lambda m: optim.AdamW(two_groups(m)), True),
                         ("factorized_amd.optim.Adam, flat gradients (a third time)", lambda m: optim.Adam(m.parameters()), True)):
    import gc
    model = optimizer = None
    gc.collect(); torch.cuda.empty_cache()
    model = MFM_KL_EF(*cfgs)
    optimizer = make(model)
    model = model.to("cuda")
    model.train()
    print("%-78s %.3f ms/step" % (name, timed_steps(lambda k: loop(model, optimizer, k, item), 300, 30)))
model = MFM_KL_EF(*cfgs).to("cuda")
print("%-70s %.3f ms/step" % ("model.engine.train_step(X, y)  (one C call)",
                              timed(lambda: model.engine.train_step(X, y), 300, 30)))

# eager, the other two classes of train_mfm (fused plan forward / backward since round 3 / 4)
from factorized_amd import mfm_model as M2
for cls_name in ("MFM_KL", "MFM"):
    model = getattr(M2, cls_name)(*cfgs)
    optimizer = optim.Adam(model.parameters())
    model = model.to("cuda")
    model.train()
    print("%-70s %.3f ms/step" % ("factorized_amd.optim.Adam, flat gradients, %s" % cls_name,
                                  timed_steps(lambda k: loop(model, optimizer, k, True), 300, 30)))

# the same loop captured once into a hipGraph (train.GraphedModuleStep: fused plan with device-side epochs / dropout streams,
# optim.Adam(capturable=True)) and replayed; per-step input copy into the static batch included
from factorized_amd import train
for cls_name in ("MFM_KL_EF", "MFM_KL", "MFM"):
    from factorized_amd import mfm_model as M
    model = getattr(M, cls_name)(*cfgs).to("cuda")
    model.train()
    gs = train.GraphedModuleStep(model, config, B, T, lr=1e-3)
    print("%-70s %.3f ms/step" % ("GraphedModuleStep(%s): the unchanged loop as one hipGraph replay" % cls_name,
                                  timed(lambda: gs.step(X, y), 300, 30)))
    assert float(gs.loss) == float(gs.loss) and model.engine.check_status() == 0

if os.environ.get("MFM_DROPIN_PROFILE"):
    import cProfile, pstats
    model = MFM_KL_EF(*cfgs)
    optimizer = optim.Adam(model.parameters())
    model = model.to("cuda"); model.train()
    loop(model, optimizer, 30, False)
    torch.cuda.synchronize()
    pr = cProfile.Profile()
    pr.enable()
    loop(model, optimizer, 300, False)
    torch.cuda.synchronize()
    pr.disable()
    st = pstats.Stats(pr)
    st.sort_stats("cumulative").print_stats(45)

if os.environ.get("MFM_DROPIN_SECTIONS"):
    model = MFM_KL_EF(*cfgs)
    optimizer = optim.Adam(model.parameters())
    model = model.to("cuda"); model.train()
    criterion, gen_criterion = nn.L1Loss(), nn.MSELoss()
    acc = [0.0] * 5
    pc = time.perf_counter
    for it in range(330):
        t0 = pc()
        optimizer.zero_grad()
        t1 = pc()
        decoded, mmd_loss, missing_loss = model.forward(X)
        t2 = pc()
        [x_l_hat, x_a_hat, x_v_hat, y_hat] = decoded
        gen_loss = config["lda_xl"] * gen_criterion(x_l_hat, X[:, :, :d_l]) + config["lda_xa"] * gen_criterion(x_a_hat, X[:, :, d_l:d_l + d_a]) \
            + config["lda_xv"] * gen_criterion(x_v_hat, X[:, :, d_l + d_a:])
        disc_loss = criterion(y_hat.squeeze(1), y)
        loss = disc_loss + gen_loss + config["lda_mmd"] * mmd_loss + missing_loss
        t3 = pc()
        loss.backward()
        t4 = pc()
        optimizer.step()
        t5 = pc()
        if it >= 30:
            for k, d in enumerate((t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                acc[k] += d
        if it % 50 == 49:
            torch.cuda.synchronize()
    print("host us/step: zero_grad %.0f  forward %.0f  loss ops %.0f  backward %.0f  step %.0f  (sum %.0f)" %
          tuple([1e6 * a / 300 for a in acc] + [1e6 * sum(acc) / 300]))
