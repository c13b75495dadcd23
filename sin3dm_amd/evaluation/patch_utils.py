"""The geometry metrics of the reference's evaluation/patch_utils.py on the device (s3d_eval.hip): LP-IoU,
LP-F-score and the pairwise-IoU diversity, from the voxel grids the decoders and data.mesh_sampler write.

Occupancy is bit-packed and every metric is computed from integer counts; the float32 expressions are the reference's, in its
order, so the per-patch maxima carry the reference's bits.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import random
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib

SEED = 1234                      # the reference seeds python's global stream with it (eval_LP_given_paths :126)


def _dims(shape):
    return (C.c_int * 3)(*[int(s) for s in shape])


def _as_occupancy(vox):
    """A device uint8 [H][W][D] occupancy, non-zero = occupied."""
    _lib.require_gpu(vox)
    assert vox.dim() == 3, f"a volume is [H][W][D], got {tuple(vox.shape)}"
    return (vox if vox.dtype == torch.uint8 else (vox != 0).to(torch.uint8)).contiguous()


# ------------------------------------------------------------------ loaders
def pooled_shape(shape, resolution):
    """The reference's target shape (:13, :25): the longest axis becomes `resolution`."""
    return tuple(int(x * resolution / max(shape)) for x in shape)


def pool_occupancy(vox, out_shape):
    """OR over the adaptive-pooling windows: F.adaptive_max_pool3d of an occupancy."""
    vox = _as_occupancy(vox)
    out = torch.empty(tuple(int(s) for s in out_shape), dtype=torch.uint8, device=vox.device)
    _lib.check(_lib.load().s3d_eval_pool_or(_lib.ptr(vox), _dims(vox.shape), _dims(out.shape), _lib.ptr(out), _lib.stream_ptr()))
    return out


def _to_resolution(occ, resolution):
    if max(occ.shape) != resolution:
        occ = pool_occupancy(occ, pooled_shape(occ.shape, resolution))
    return occ.bool()


def load_voxgrid(path, resolution=128, device="cuda"):
    """A generated shape's occupancy (reference :21): key `vox_grid` (voxel.npz of decode_mesh / decode_texmesh), else `voxel`
    (r{reso}_voxel.npz of decode_voxel); both hold sdf < 0."""
    _lib.require_gpu()
    with np.load(path) as f:
        key = "vox_grid" if "vox_grid" in f.files else "voxel"
        if key not in f.files:
            raise KeyError(f"{path}: neither 'vox_grid' nor 'voxel' in {f.files}")
        vox = np.ascontiguousarray(f[key])
    return _to_resolution((torch.from_numpy(vox).to(device) != 0).to(torch.uint8), resolution)


def load_sdfgrid2vox(path, resolution=128, device="cuda"):
    """The training shape's occupancy (reference :8): `sdf_grid` of data.mesh_sampler, occupied where float32(sdf) <= 0.
    Min-pooling the SDF and then testing <= 0 is OR-pooling this mask."""
    _lib.require_gpu()
    with np.load(path) as f:
        sdf = np.ascontiguousarray(f["sdf_grid"])
    return _to_resolution((torch.from_numpy(sdf).float().to(device) <= 0).to(torch.uint8), resolution)


# ------------------------------------------------------------------ patches
def n_words(patch_size):
    return (patch_size ** 3 + 63) // 64


def candidate_counts(shape, patch_size, stride=None):
    """Candidate patches per axis of the volume zero-padded by patch_size // 2; validates patch_size and stride."""
    stride = patch_size // 2 if stride is None else stride
    counts = (C.c_int * 3)()
    _lib.check(_lib.load().s3d_eval_patch_counts(_dims(shape), int(patch_size), int(stride), counts))
    return tuple(counts)


def patch_validity(vox, patch_size, stride=None):
    """uint8 flags of all candidates in row-major (a, b, c) order: the centre cube holds an occupied and a free voxel."""
    vox = _as_occupancy(vox)
    stride = patch_size // 2 if stride is None else stride
    na, nb, nc = candidate_counts(vox.shape, patch_size, stride)
    flags = torch.empty(na * nb * nc, dtype=torch.uint8, device=vox.device)
    _lib.check(_lib.load().s3d_eval_patch_valid(_lib.ptr(vox), _dims(vox.shape), int(patch_size), int(stride), _lib.ptr(flags),
                                                _lib.stream_ptr()))
    return flags


def pack_patches(vox, patch_size, stride, indices, word_major=False):
    """(words, counts) of the listed candidates: int64 bit patterns [n][n_words] (or [n_words][n]), int32 population counts."""
    vox = _as_occupancy(vox)
    indices = indices.to(device=vox.device, dtype=torch.int64).contiguous()
    n, nw = indices.numel(), n_words(patch_size)
    words = torch.empty((nw, n) if word_major else (n, nw), dtype=torch.int64, device=vox.device)
    counts = torch.empty(n, dtype=torch.int32, device=vox.device)
    _lib.check(_lib.load().s3d_eval_pack_patches(_lib.ptr(vox), _dims(vox.shape), int(patch_size), int(stride), _lib.ptr(indices), n,
                                                 int(word_major), _lib.ptr(words), _lib.ptr(counts), _lib.stream_ptr()))
    return words, counts


@dataclass
class Patches:
    """The valid patches of one volume, in the reference's order.  words: int64 bit patterns, [n][n_words] or, word-major,
    [n_words][n]; counts: int32 [n]; indices: int64 [n], the candidates' positions in the row-major candidate grid."""
    words: torch.Tensor
    counts: torch.Tensor
    indices: torch.Tensor
    patch_size: int
    word_major: bool = False

    def __len__(self):
        return int(self.counts.numel())

    def select(self, chosen):
        """The patches at positions `chosen` (any order, as gen_patches[indices] in the reference)."""
        chosen = torch.as_tensor(chosen, dtype=torch.int64, device=self.counts.device)
        return Patches(self.words.index_select(1 if self.word_major else 0, chosen).contiguous(), self.counts[chosen].contiguous(),
                       self.indices[chosen].contiguous(), self.patch_size, self.word_major)

    def to_layout(self, word_major):
        if bool(word_major) == self.word_major:
            return self
        return Patches(self.words.t().contiguous(), self.counts, self.indices, self.patch_size, bool(word_major))


def extract_valid_patches(vox, patch_size, stride=None, word_major=False):
    """extract_valid_patches_unfold (:46) without the unfold: validity flags, order-preserving compaction (torch), packing."""
    vox = _as_occupancy(vox)
    stride = patch_size // 2 if stride is None else stride
    indices = torch.nonzero(patch_validity(vox, patch_size, stride)).view(-1)
    words, counts = pack_patches(vox, patch_size, stride, indices, word_major)
    return Patches(words, counts, indices, int(patch_size), bool(word_major))


# ------------------------------------------------------------------ metrics
def lp_maxima(gen, ref):
    """Per generated patch: the largest IoU and the largest F-score over the reference patches (float32 [n_gen] each)."""
    assert gen.patch_size == ref.patch_size, (gen.patch_size, ref.patch_size)
    gen, ref = gen.to_layout(False), ref.to_layout(True)
    dev = gen.counts.device
    max_iou = torch.empty(len(gen), dtype=torch.float32, device=dev)            # the entry point zeroes them before the merge
    max_f = torch.empty(len(gen), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().s3d_eval_lp_max(_lib.ptr(gen.words), _lib.ptr(gen.counts), len(gen), _lib.ptr(ref.words), _lib.ptr(ref.counts),
                                           len(ref), n_words(gen.patch_size), _lib.ptr(max_iou), _lib.ptr(max_f), _lib.stream_ptr()))
    return max_iou, max_f


def lp_metrics(gen, ref, threshold=0.95):
    """eval_LP_IoU and eval_LP_Fscore (:77, :100) in one pass.  No generated patch: the averages and percents are NaN."""
    max_iou, max_f = lp_maxima(gen, ref)
    n = len(gen)
    if n == 0:
        iou_avg = iou_percent = f_avg = f_percent = float("nan")
    else:                                                            # one copy to the host for the four numbers (counts < 2^24: exact)
        iou_avg, f_avg, iou_over, f_over = torch.stack([torch.mean(max_iou), torch.mean(max_f), (max_iou > threshold).sum().float(),
                                                        (max_f > threshold).sum().float()]).tolist()
        iou_percent, f_percent = int(iou_over) * 1.0 / n, int(f_over) * 1.0 / n
    return dict(iou_avg=iou_avg, iou_percent=iou_percent, f_avg=f_avg, f_percent=f_percent, max_iou=max_iou, max_f=max_f)


def pairwise_counts(vols):
    """int64 [N][N] intersection and union counts of N equally shaped volumes."""
    vols = torch.stack([_as_occupancy(v) for v in vols]) if not torch.is_tensor(vols) else vols
    _lib.require_gpu(vols)
    vols = (vols if vols.dtype == torch.uint8 else (vols != 0).to(torch.uint8)).contiguous()
    n = vols.shape[0]
    voxels = vols[0].numel() if n else 1
    nw = (voxels + 63) // 64
    lib = _lib.load()
    words = torch.empty((n, nw), dtype=torch.int64, device=vols.device)
    inter = torch.empty((n, n), dtype=torch.int64, device=vols.device)
    union = torch.empty((n, n), dtype=torch.int64, device=vols.device)
    _lib.check(lib.s3d_eval_pack_volumes(_lib.ptr(vols), n, voxels, _lib.ptr(words), _lib.stream_ptr()))
    _lib.check(lib.s3d_eval_pairwise_counts(_lib.ptr(words), n, nw, _lib.ptr(inter), _lib.ptr(union), _lib.stream_ptr()))
    return inter, union


def pairwise_iou_dist(vols):
    """pairwise_IoU_dist (:30): the mean over i of the float32 mean over j != i of 1 - inter / union."""
    inter, union = pairwise_counts(vols)
    n = inter.shape[0]
    dist = 1.0 - inter / union                                       # int64 / int64: float32, as in the reference
    off = ~torch.eye(n, dtype=torch.bool, device=dist.device)
    rows = dist[off].view(n, n - 1).mean(dim=1)
    return float(np.mean(rows.cpu().numpy().astype(np.float64)))


# ------------------------------------------------------------------ drivers
def shuffled_choice(rng, n_valid, patch_num):
    """The reference's sampling (:144-146) on a private stream: shuffle range(n_valid), keep the first patch_num."""
    indices = list(range(n_valid))
    rng.shuffle(indices)
    return indices[:patch_num]


def eval_lp(paths, ref_path, patch_size=11, stride=5, patch_num=1000, resolution=128):
    """eval_LP_given_paths (:125).  One random.Random(1234) serves all shapes in turn: the permutations of random.seed(1234)
    without touching the caller's global stream."""
    rng = random.Random(SEED)
    ref = extract_valid_patches(load_sdfgrid2vox(ref_path, resolution=resolution), patch_size, stride, word_major=True)
    rows = []
    for path in paths:
        gen = extract_valid_patches(load_voxgrid(path, resolution=resolution), patch_size, stride)
        gen = gen.select(shuffled_choice(rng, len(gen), patch_num))
        m = lp_metrics(gen, ref)
        rows.append((m["iou_avg"], m["iou_percent"], m["f_avg"], m["f_percent"]))
    means = [float(np.mean(c).round(6)) for c in zip(*rows)] if rows else [float("nan")] * 4
    return {"LP-IOU-avg": means[0], "LP-IOU-percent": means[1], "LP-F-score-avg": means[2], "LP-F-score-percent": means[3]}


def eval_div(paths, resolution=128):
    """eval_Div_given_paths (:169)."""
    vols = torch.stack([load_voxgrid(p, resolution=resolution) for p in paths], dim=0)
    return {"Div": float(np.float64(pairwise_iou_dist(vols)).round(6))}
