"""Expected values of the zeroed-modality test protocol (reference mfm_mosi.py:572-596) from the CPU oracle, shared by
test_zeros_host.py and test_gpu_zeros.py: the batch through oracle.mfm_oracle three times, modality l, a, v zeroed in turn."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mfm_oracle as O


def bounds(cfg):
    d_l, d_a, d_v = cfg["input_dims"]
    return ((0, d_l), (d_l, d_l + d_a), (d_l + d_a, d_l + d_a + d_v))


def zeroed(x, cfg, c):
    """a copy of x [T, N, D] (tensor or ndarray) with the columns of modality c set to zero"""
    a, b = bounds(cfg)[c]
    xz = x.clone() if torch.is_tensor(x) else x.copy()
    xz[:, :, a:b] = 0
    return xz


def oracle_zeros(variant, cfgs, weights, xn, yn=None, gauss=None, double=False):
    """-> dict(y_hat [3, N, od] float32, gen [3], disc [3] or None) in float64 where scalar, from the oracle in eval mode;
    `double`: the oracle itself computes in float64 (the default is its fp32 forward)"""
    cfg = cfgs[0]
    m = O.build(variant, cfgs)
    O.load_numpy_weights(m, weights)
    m.eval()
    if gauss is not None:
        m.mmd_gauss = gauss
    torch.set_num_threads(4)
    x = torch.from_numpy(np.ascontiguousarray(xn))
    if double:
        m, x = m.double(), x.double()
    y = None if yn is None else torch.from_numpy(np.ascontiguousarray(yn))
    ce = cfg.get("loss", "l1") == "ce"
    y_hat, gen, disc = [], [], []
    with torch.no_grad():
        for c, (a, b) in enumerate(bounds(cfg)):
            decoded, _, _ = m.forward(zeroed(x, cfg, c))
            yh = decoded[3]
            y_hat.append(yh.numpy().astype(np.float32))
            gen.append(float(F.mse_loss(decoded[c].double(), x[:, :, a:b].double())))
            if y is not None:
                if ce:
                    disc.append(float(F.cross_entropy(yh.double(), y)))
                else:
                    disc.append(float(F.l1_loss(yh.double().reshape(-1), y.double().reshape(-1))))
    return dict(y_hat=np.stack(y_hat), gen=np.array(gen), disc=np.array(disc) if y is not None else None)
