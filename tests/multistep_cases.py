"""Float64 restatements and case tables for the DPM-Solver++ multistep sampler, shared by
test_multistep_host.py and test_multistep_gpu.py.  Nothing here touches a GPU.

The restatement of the coefficients is written from the levels (alpha, sigma, lambda per kept step), not from the product code's
running expressions, and can be asked to make one of the mistakes the product code could make (FAULTS): the host test shows that
the comparison it uses would catch each."""
import numpy as np

# the float64 comparison of the product tables with the restatement: both evaluate the same formulas in another order, the values are
# O(1) (|c| <= 3.1 on the spacings used) and a handful of float64 operations deep: 1e-12 leaves four digits of room over the few
# 1e-16 measured and is ten orders below the smallest injected fault
TABLE_TOL = 1e-12

FAULTS = ("c1_sign", "r_inverted", "h_wrong_step", "order2_at_0")


def levels(diff):
    """(alpha, sigma, lambda) of the levels 0 .. T of a schedule: entry 0 is clean data (alpha 1, sigma 0, lambda +inf), entry
    i + 1 is the level of index i."""
    ac = np.concatenate([[1.0], np.asarray(diff.alphas_cumprod, dtype=np.float64)])
    with np.errstate(divide="ignore"):
        lam = 0.5 * (np.log(ac) - np.log1p(-ac))
    return np.sqrt(ac), np.sqrt(1.0 - ac), lam


def restated_tables(diff, order=2, sde=False, fault=None):
    """[4][T] float64 (cx, c0, c1, cn) and the per-index orders.  Index i steps from level i + 1 down to level i."""
    assert fault in (None,) + FAULTS
    alpha, sigma, lam = levels(diff)
    T = diff.num_timesteps
    tab, orders = np.zeros((4, T)), np.ones(T, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(T):
            s, t = i + 1, i
            if i == 0 and fault != "order2_at_0":
                tab[:, i] = (0.0, 1.0, 0.0, 0.0)
                continue
            h = lam[t] - lam[s]
            if fault == "h_wrong_step" and i < T - 1:
                h = lam[s] - lam[s + 1]
            e1 = np.exp(-h)
            if sde:
                cx, g, cn = sigma[t] / sigma[s] * e1, alpha[t] * (1.0 - e1 * e1), sigma[t] * np.sqrt(1.0 - e1 * e1)
            else:
                cx, g, cn = sigma[t] / sigma[s], alpha[t] * (1.0 - e1), 0.0
            if order == 2 and i < T - 1:
                r = (lam[s] - lam[s + 1]) / (lam[t] - lam[s])
                if fault == "r_inverted":
                    r = 1.0 / r
                c1 = -g / (2.0 * r)
                tab[:, i] = (cx, g - c1, -c1 if fault == "c1_sign" else c1, cn)
                orders[i] = 2
            else:
                tab[:, i] = (cx, g, 0.0, cn)
    return tab, orders


# ------------------------------------------------------------------ the Gaussian case with a closed-form answer
DATA_VAR = 0.25             # data ~ N(0, 0.25): the optimal x0-predictor is linear in x_t and the probability-flow ODE has a closed form


def gaussian_error(diff, order, tables=None):
    """|x - exact| at the end of the trajectory (the level of index 0, i.e. after the step of index 1) of the multistep ODE solver run
    with the product code's coefficients on a scalar state in float64, from x_T = 1 with the optimal predictor
    x0(x, level) = alpha v / (alpha^2 v + sigma^2) x.  exact: the ODE keeps x / sqrt(alpha^2 v + sigma^2) constant."""
    tab, orders = tables if tables is not None else diff.multistep_tables(order=order, sde=False)
    ac = np.asarray(diff.alphas_cumprod, dtype=np.float64)
    std = lambda q: np.sqrt(q * DATA_VAR + 1.0 - q)
    x, x0_prev, at0 = 1.0, 0.0, None
    for i in range(diff.num_timesteps - 1, -1, -1):
        al = np.sqrt(ac[i])
        x0 = al * DATA_VAR / (al * al * DATA_VAR + 1.0 - ac[i]) * x
        x = tab[0, i] * x + tab[1, i] * x0 + (tab[2, i] * x0_prev if orders[i] == 2 else 0.0)
        x0_prev = x0
        if i == 1:
            at0 = x
    return abs(at0 - std(ac[0]) / std(ac[-1]))


# ------------------------------------------------------------------ GPU cases (the shapes of tests/test_edit_gpu.py: the smallest that reach each path)
# name: (model channels, latent channels, B, (H, W, D))
CONFIGS = {"standalone32": (32, 12, 2, (10, 14, 6)),        # the two-kernel path (the pixel-chunk head does not take 32 channels)
           "fused_odd": (64, 12, 1, (12, 9, 7)),            # fused, odd sizes, line tails shorter than 64
           "fused_tail": (64, 12, 2, (2, 2, 47)),           # fused, the corner's tail loop
           "fused_geo": (64, 4, 2, (12, 9, 7)),             # geometry-only width
           "fused_cq32": (128, 12, 1, (12, 9, 7))}          # the CQ = 32 instantiation
# (the 256-channel instantiation, CQ = 64, is covered by tests/test_multistep_resources.py only)


def synthetic_tables(T):
    """[4][T] float32 with all four rows non-trivial at every index, index 0 included (the schedule's own tables never exercise
    c1 and cn together there)."""
    i = np.arange(T, dtype=np.float64)
    return np.stack([0.9 - 0.01 * i, 0.3 + 0.02 * i, -0.45 + 0.005 * i, 0.2 + 0.003 * i]).astype(np.float32)
