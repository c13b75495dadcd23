"""The cases of the SIFID / LPIPS tests and a float64 restatement of the reference's computation, shared by
tests/test_imgmetrics_host.py, tests/test_imgmetrics_gpu.py and the fixture generator tests/golden/make_golden_imgmetrics.py.
Weights and images come from seeds and formulas; only the 1152 linear LPIPS weights are read from the fixture.

The restatement is written from the text of evaluation/sifid.py, evaluation/inception.py and evaluation/lpips.py and
torchvision's module definitions (BasicConv2d, AlexNet.features); tests/golden/imgmetrics.npz pins it to the reference's modules.
"""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from ssfid_cases import bound, check_tail  # noqa: F401  (the tolerances of DESIGN.md §21, kept for §23)

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (64, 192)
# name, Cin, Cout, k, stride, pad, pool in front
STEM = (("Conv2d_1a_3x3", 3, 32, 3, 2, 0, False), ("Conv2d_2a_3x3", 32, 32, 3, 1, 0, False), ("Conv2d_2b_3x3", 32, 64, 3, 1, 1, False),
        ("Conv2d_3b_1x1", 64, 80, 1, 1, 0, True), ("Conv2d_4a_3x3", 80, 192, 3, 1, 0, False))
ALEX = (("features.0", 3, 64, 11, 4, 2, False), ("features.3", 64, 192, 5, 1, 2, True), ("features.6", 192, 384, 3, 1, 1, True),
        ("features.8", 384, 256, 3, 1, 1, False), ("features.10", 256, 256, 3, 1, 1, False))
LPIPS_MU, LPIPS_SIGMA = (-0.03, -0.088, -0.188), (0.458, 0.448, 0.450)

# image name: (H, W, seed).  a*: the batch of three equal-size images (also the LPIPS group and the end-to-end tree)
IMAGES = {
    "a0": (96, 80, 1), "a1": (96, 80, 2), "a2": (96, 80, 3),   # stem 45 x 37 (odd pre-pool extents), 320 rows at dims 192
    "b": (98, 101, 4), "b1": (98, 101, 5),                     # stem 46 x 48: the pool leaves a row and a column unused; AlexNet 23 x 24 -> 11 x 11 -> 5 x 5
    "c": (75, 101, 6), "c1": (75, 101, 7),                     # a second non-square shape
    "d": (200, 136, 8), "d1": (200, 136, 9),                   # 6305 rows: several tiles both ways, several Gram blocks
    "s": (40, 40, 10), "s1": (40, 40, 11),                     # 36 rows for 192 channels: a singular covariance; too small for AlexNet
}
PARITY = ("a0", "a1", "a2", "b", "b1", "c", "c1", "d", "d1")   # rows > C, no constant channel (asserted by the generator)
BATCH = ("a0", "a1", "a2")
SIFID_PAIRS = {"pa": ("a0", "a1"), "pa2": ("a0", "a2"), "pb": ("b", "b1"), "pc": ("c", "c1"), "pd": ("d", "d1")}
SINGULAR_PAIR = ("s", "s1")
LPIPS_PAIRS = {"pa": ("a0", "a1"), "pa2": ("a0", "a2"), "pa12": ("a1", "a2"), "pb": ("b", "b1"), "pc": ("c", "c1"), "pd": ("d", "d1")}
ACT_CASE = "a0"                          # the image whose activations the fixture stores
E2E_VIEWS = 2                            # the end-to-end tree: two views of two sizes, three generated samples; sample_2 repeats renders
E2E_TREE = {"ref": ("a0", "b"), "gen": (("a1", "b1"), ("a2", "b"), ("a0", "b1"))}


@functools.lru_cache(maxsize=None)
def image(name):
    """uint8 RGBA [H][W][4]: smooth colour fields, edges and per-pixel noise, every sample value reachable; alpha is a disc."""
    H, W, seed = IMAGES[name]
    rng = np.random.Generator(np.random.PCG64([seed, 0x1396]))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W, 4), dtype=np.uint8)
    for c in range(3):
        f = rng.uniform(0.02, 0.25, size=4)
        ph = rng.uniform(0, 6.28, size=2)
        v = 0.5 + 0.3 * np.sin(f[0] * x + f[1] * y + ph[0]) + 0.2 * np.sign(np.sin(f[2] * x - f[3] * y + ph[1]))
        v = v + rng.normal(0.0, 0.08, size=(H, W))
        out[..., c] = np.clip(np.rint(v * 255.0), 0, 255).astype(np.uint8)
    out[..., 3] = np.where((x - W / 2) ** 2 + (y - H / 2) ** 2 < (0.45 * min(H, W)) ** 2, 255, 0)
    out.setflags(write=False)
    return out


def _coarse(a):
    """Rounded to 8 significant bits: what a calibration pass found, insensitive to the last bits of that pass."""
    m, e = np.frexp(np.asarray(a, dtype=np.float64))
    return np.ldexp(np.rint(m * 256.0) / 256.0, e)


@functools.lru_cache(maxsize=None)
def inception_weights():
    """Procedural stem weights (float32 tensors by torchvision's names).  The BatchNorm running statistics come from a float64
    calibration pass over image a0, rounded coarsely, so that every unit's output is roughly standardised before its affine and no
    channel is dead; with plain random statistics about 45 of Conv2d_4a_3x3's channels are, their inputs being all positive."""
    rng = np.random.Generator(np.random.PCG64([11, 0x51F1D]))
    w = {}
    x = sifid_input(image("a0")).double()
    for name, cin, cout, k, stride, pad, pool in STEM:
        cw = (rng.standard_normal((cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
        gamma = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        beta = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
        if pool:
            x = F.max_pool2d(x, 3, 2)
        y = F.conv2d(x, torch.from_numpy(cw).double(), stride=stride, padding=pad)
        mean = _coarse(y.mean(dim=(0, 2, 3)).numpy()).astype(np.float32)
        var = _coarse(y.var(dim=(0, 2, 3), unbiased=False).numpy()).astype(np.float32)
        for key, val in ((".conv.weight", cw), (".bn.weight", gamma), (".bn.bias", beta), (".bn.running_mean", mean), (".bn.running_var", var)):
            w[name + key] = torch.from_numpy(val)
        x = F.relu(F.batch_norm(y, torch.from_numpy(mean).double(), torch.from_numpy(var).double(), torch.from_numpy(gamma).double(),
                                torch.from_numpy(beta).double(), False, 0.0, 1e-3))
    return w


@functools.lru_cache(maxsize=None)
def alexnet_weights():
    """Procedural AlexNet `features` weights: He-scaled, small positive biases.  The last convolution is scaled by 1e-5, so that
    sum_c x^2 of the fifth map is about 1e-8 and the 1e-10 under the root of normalize() moves that map's term by parts in a
    thousand: x * rsqrt(sum + eps) and x / (sqrt(sum) + eps) agree to round-off on maps of ordinary size."""
    rng = np.random.Generator(np.random.PCG64([12, 0xA1E7]))
    w = {}
    for name, cin, cout, k, _, _, _ in ALEX:
        s = 1e-5 if name == "features.10" else 1.0
        w[name + ".weight"] = torch.from_numpy((rng.standard_normal((cout, cin, k, k)) * (s * np.sqrt(2.0 / (cin * k * k)))).astype(np.float32))
        w[name + ".bias"] = torch.from_numpy((rng.uniform(0.0, 0.1, cout) * s).astype(np.float32))
    return w


@functools.lru_cache(maxsize=None)
def lpips_linear():
    """The reference's 1152 linear LPIPS weights, {lpips_weights.<l>.main.1.weight: [1][C][1][1]}, from the fixture."""
    g = np.load(os.path.join(HERE, "golden", "imgmetrics.npz"))
    return {f"lpips_weights.{l}.main.1.weight": torch.from_numpy(np.asarray(g[f"lin/{l}"], dtype=np.float32).reshape(1, -1, 1, 1)) for l in range(5)}


def sifid_input(img, fault=None):
    """float32 [1][3][H][W]: matplotlib's imread (float32 u8 / 255), RGB of RGBA, then InceptionV3's 2 x - 1 in float32."""
    x = np.asarray(img)[..., :3].astype(np.float32) / np.float32(255.0)
    t = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]
    return t if fault == "no_2x1" else 2 * t - 1


def lpips_input(img, fault=None):
    """float32 [1][3][H][W]: PIL RGB / 255. and (v - 0.5) / 0.5 in float64, the cast to float32, then (x - mu) / sigma in float32."""
    v = (np.asarray(img)[..., :3] / 255. - 0.5) / 0.5
    t = torch.from_numpy(np.ascontiguousarray(v.transpose(2, 0, 1))).type(torch.FloatTensor)[None]
    if fault == "no_imagenet":
        return t
    return (t - torch.tensor(LPIPS_MU).view(1, 3, 1, 1)) / torch.tensor(LPIPS_SIGMA).view(1, 3, 1, 1)


def _rows(a):
    return a[0].permute(1, 2, 0).reshape(-1, a.shape[1]).numpy()


def sifid_restate(img, w, dims, fault=None):
    """Float64: ([per-unit activations [H'][W'][C]], mu [C], sigma [C][C]).  fault: None, 'bn_eps' (1e-5 instead of 1e-3),
    'ceil_pool', 'ddof0', 'no_2x1'."""
    x = sifid_input(img, fault).double()
    acts = []
    for name, _, _, _, stride, pad, pool in STEM[:3 if dims == 64 else 5]:
        if pool:
            x = F.max_pool2d(x, 3, 2, ceil_mode=fault == "ceil_pool")
        x = F.conv2d(x, w[name + ".conv.weight"].double(), stride=stride, padding=pad)
        x = F.relu(F.batch_norm(x, w[name + ".bn.running_mean"].double(), w[name + ".bn.running_var"].double(), w[name + ".bn.weight"].double(),
                                w[name + ".bn.bias"].double(), False, 0.0, 1e-5 if fault == "bn_eps" else 1e-3))
        acts.append(x[0].permute(1, 2, 0).numpy())
    rows = _rows(x)
    return acts, np.mean(rows, axis=0), np.cov(rows, rowvar=False, ddof=0 if fault == "ddof0" else 1)


def alexnet_maps(x, w):
    """The five post-ReLU maps [1][C][H'][W'] of AlexNet's features in the dtype of x; raises where the final pool would be empty."""
    maps = []
    for name, _, _, _, stride, pad, pool in ALEX:
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w[name + ".weight"].to(x.dtype), w[name + ".bias"].to(x.dtype), stride=stride, padding=pad))
        maps.append(x)
    F.max_pool2d(x, 3, 2)
    return maps


def lpips_restate(img_a, img_b, w, lin, fault=None):
    """Float64: (the five per-map terms, their sum, image a's maps [H'][W'][C]).  fault: None, 'sqrt_eps' (x / (sqrt(sum) + eps)),
    'no_imagenet'."""
    def unit(m):
        s = torch.sum(m ** 2, dim=1, keepdim=True)
        return m / (torch.sqrt(s) + 1e-10) if fault == "sqrt_eps" else m * torch.rsqrt(s + 1e-10)
    ma, mb = alexnet_maps(lpips_input(img_a, fault).double(), w), alexnet_maps(lpips_input(img_b, fault).double(), w)
    terms = []
    for l, (a, b) in enumerate(zip(ma, mb)):
        lw = lin[f"lpips_weights.{l}.main.1.weight"].double()
        terms.append(float(torch.mean(F.conv2d((unit(a) - unit(b)) ** 2, lw))))
    return np.asarray(terms), float(np.sum(terms)), [m[0].permute(1, 2, 0).numpy() for m in ma]


@functools.lru_cache(maxsize=None)
def sifid_restated(name, dims):
    """The unfaulted restatement of a named image, computed once per process and shared; do not write to the arrays."""
    acts, mu, sigma = sifid_restate(image(name), inception_weights(), dims)
    for a in acts + [mu, sigma]:
        a.setflags(write=False)
    return acts, mu, sigma


@functools.lru_cache(maxsize=None)
def lpips_restated(a, b):
    return lpips_restate(image(a), image(b), alexnet_weights(), lpips_linear())


def write_tree(root):
    """The end-to-end tree of PNGs: root/ref/renderings/00i.png and root/src/sample_j/renderings/00i.png; returns (gen dirs, ref dir)."""
    from sin3dm_amd.encoding.isosurface import png_bytes

    def put(d, names):
        os.makedirs(d)
        for i, n in enumerate(names):
            with open(os.path.join(d, f"{i:03d}.png"), "wb") as fh:
                fh.write(png_bytes(image(n)))
        return d
    ref = put(os.path.join(root, "ref", "renderings"), E2E_TREE["ref"])
    gen = [put(os.path.join(root, "src", f"sample_{j}", "renderings"), names) for j, names in enumerate(E2E_TREE["gen"])]
    return gen, ref
