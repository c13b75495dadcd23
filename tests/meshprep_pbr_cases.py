"""Restatement, border mask and images of the PBR mesh-preprocessing tests (tests/test_meshprep_pbr_host.py,
test_meshprep_pbr_gpu.py; DESIGN.md §16 "PBR variant").  NumPy only: nothing here needs a GPU.

texels8 restates s3d_meshsdf_texture_pbr in float64 and integers.  The device interpolates the uv in float32; the two agree
wherever the float64 texel coordinate is not within rounding of a half-integer, which near_border flags with a margin of 1e-3 of
a texel (float32 rounding of u (W - 1) with W <= 16 is below 4e-6).  `python tests/meshprep_pbr_cases.py` prints the share of the
shared query set that near_border leaves out (CPU only)."""
import numpy as np

FIELDS = ("image", "metallic_image", "roughness_image", "normal_image")          # albedo, metallic, roughness, normal
CHANNELS = (3, 1, 1, 3)
COLUMNS = ((0, 3), (3, 4), (4, 5), (5, 8))                                        # where each map lands in a row of eight
FLAT_NORMAL = np.array([128, 128, 255], dtype=np.uint8)
BORDER = 1e-3
N_QUERIES, BORDER_CAP = 6000, 0.02


# ------------------------------------------------------------------ images whose texels encode their own (x, y) and a map id
def coded_rgb(W, H, map_id):
    """uint8 [H, W, 3]: (16 x + id, 16 y + id, 200 + id); W, H <= 16, id < 16.  No texel equals another one's, or another map's."""
    assert W <= 16 and H <= 16 and 0 <= map_id < 16
    img = np.empty((H, W, 3), dtype=np.uint8)
    img[..., 0] = np.arange(W)[None, :] * 16 + map_id
    img[..., 1] = np.arange(H)[:, None] * 16 + map_id
    img[..., 2] = 200 + map_id
    return img


def coded_plane(W, H, map_id):
    """uint8 [H, W]: 4 (y W + x) + id; W H <= 64, id < 4."""
    assert W * H <= 64 and 0 <= map_id < 4
    return ((np.arange(H)[:, None] * W + np.arange(W)[None, :]) * 4 + map_id).astype(np.uint8)


def material0():
    """The four maps of different sizes of the shared case: albedo 16 x 8, metallic 5 x 7, roughness 7 x 5, normal 12 x 12."""
    return {"Kd": (1.0, 0.0, 1.0), "image": coded_rgb(16, 8, 1), "metallic_image": coded_plane(5, 7, 2), "roughness_image": coded_plane(7, 5, 3),
            "normal_image": coded_rgb(12, 12, 4), "Pm": 0.75, "Pr": 0.375}


def material1():
    """Scalars only."""
    return {"Kd": (0.25, 0.5, 0.125), "Pm": 0.3, "Pr": 0.7}


# ------------------------------------------------------------------ the restatement
def _plane(m, field):
    img = m.get(field)
    if img is None:
        return None
    img = np.asarray(img, dtype=np.uint8)
    if field in ("image", "normal_image"):
        return img[..., :3]
    return img[..., 0] if img.ndim == 3 else img


def query_uv(face, bary64, uvs):
    """float64 [n, 2]: the barycentric interpolation of the corner uvs, a NaN component replaced by 0 (face -1: row 0 is read, the
    caller masks it)."""
    face = np.asarray(face, dtype=np.int64)
    uv = np.einsum("nk,nkd->nd", np.asarray(bary64, dtype=np.float64), np.asarray(uvs, dtype=np.float64)[np.maximum(face, 0)])
    return np.where(np.isnan(uv), 0.0, uv)


def texel_coords(uv, W, H):
    """(tx, ty) float64: u (W - 1) and (1 - v) (H - 1), before rounding."""
    with np.errstate(invalid="ignore"):
        return uv[:, 0] * (W - 1), (1.0 - uv[:, 1]) * (H - 1)


def texels8(face, bary64, uvs, face_mat, materials, image_bytes=None):
    """float32 [n, 8] = albedo rgb | metallic | roughness | normal xyz of (face, barycentrics) pairs, by the rule and the
    fallbacks of s3d_meshsdf_texture_pbr.  materials: dicts with Kd, Pm, Pr (absent: 0) and the maps of FIELDS (absent: None).
    image_bytes: the size of the packed buffer the device is told (None: all of it); the maps are packed material by material
    in the order of FIELDS, and one that would end past image_bytes counts as absent."""
    face = np.asarray(face, dtype=np.int64)
    face_mat = np.asarray(face_mat, dtype=np.int64)
    n = len(face)
    out = np.zeros((n, 8), dtype=np.float32)
    uv = query_uv(face, bary64, uvs)
    hit = face >= 0
    mats = np.where(hit, face_mat[np.maximum(face, 0)], -1)
    off = 0
    for mi, m in enumerate(materials):
        sel = hit & (mats == mi)
        row = np.empty(8, dtype=np.float32)
        row[0:3] = np.asarray(m.get("Kd", (1.0, 1.0, 1.0)), dtype=np.float32)
        row[3], row[4] = np.float32(m.get("Pm", 0.0)), np.float32(m.get("Pr", 0.0))
        row[5:8] = FLAT_NORMAL.astype(np.float32) / np.float32(255)
        out[sel] = row
        for field, (c0, c1) in zip(FIELDS, COLUMNS):
            img = _plane(m, field)
            if img is None:
                continue
            start, off = off, off + img.size
            if image_bytes is not None and off > image_bytes:
                continue
            H, W = img.shape[:2]
            tx, ty = texel_coords(uv, W, H)
            fx, fy = np.rint(tx), np.rint(ty)                        # half to even
            with np.errstate(invalid="ignore"):
                ok = sel & (np.abs(fx) < 1e9) & (np.abs(fy) < 1e9)   # False on a NaN (inf * 0) and on a runaway coordinate
            x, y = fx[ok].astype(np.int64) % W, fy[ok].astype(np.int64) % H
            out[ok, c0:c1] = img.reshape(H, W, -1)[y, x].astype(np.float32) / np.float32(255)
    return out


def near_border(face, bary64, uvs, face_mat, materials):
    """bool [n]: the float64 texel coordinate of some present map of the query's material is within BORDER of a half-integer."""
    face = np.asarray(face, dtype=np.int64)
    face_mat = np.asarray(face_mat, dtype=np.int64)
    uv = query_uv(face, bary64, uvs)
    hit = face >= 0
    mats = np.where(hit, face_mat[np.maximum(face, 0)], -1)
    flag = np.zeros(len(face), dtype=bool)
    for mi, m in enumerate(materials):
        sel = hit & (mats == mi)
        for field in FIELDS:
            img = _plane(m, field)
            if img is None:
                continue
            H, W = img.shape[:2]
            for t in texel_coords(uv, W, H):
                with np.errstate(invalid="ignore"):
                    flag |= sel & (np.abs(t - np.floor(t) - 0.5) < BORDER)
    return flag


def centre_uv(x, y, W, H):
    """The uv at which the rule reads texel (x, y) of a W x H map exactly: u (W - 1) = x, (1 - v) (H - 1) = y (W = 1 or H = 1: any
    finite value does; 0.25 is returned)."""
    u = np.asarray(x, dtype=np.float64) / (W - 1) if W > 1 else np.full(np.shape(x), 0.25)
    v = 1.0 - np.asarray(y, dtype=np.float64) / (H - 1) if H > 1 else np.full(np.shape(y), 0.25)
    return np.stack(np.broadcast_arrays(u, v), -1)


# ------------------------------------------------------------------ the shared query set: drawn on the host, so that what is left out is decided there
class PbrCase:
    """The torus of meshprep_cases with uv = ((x + 1) / 2, (z + 1) / 2), material 0 (four maps) on the faces whose centroid has
    x < 0 and material 1 (scalars) on the others; N_QUERIES Dirichlet barycentrics on random faces.  The device is given float32
    uvs and barycentrics; the restatement reads the same values in float64."""

    def __init__(self):
        from meshprep_cases import case
        c = case()
        self.base = c
        tri = c.V32[c.F].astype(np.float64)
        self.face_mat = (tri.mean(1)[:, 0] >= 0).astype(np.int32)
        self.uvs32 = np.stack([(tri[..., 0] + 1) / 2, (tri[..., 2] + 1) / 2], -1).astype(np.float32)
        self.materials = [material0(), material1()]
        rng = np.random.Generator(np.random.PCG64(8))
        self.face = rng.integers(0, len(c.F), size=N_QUERIES).astype(np.int32)
        self.bary32 = rng.dirichlet(np.ones(3), size=N_QUERIES).astype(np.float32)
        args = (self.face, self.bary32.astype(np.float64), self.uvs32.astype(np.float64), self.face_mat, self.materials)
        self.expect = texels8(*args)
        self.border = near_border(*args)
        self.on0 = self.face_mat[self.face] == 0

    def sampler(self):
        from sin3dm_amd.data.mesh_sampler_pbr import MeshSamplerPBR
        c = self.base
        return MeshSamplerPBR(verts=c.V32.astype(np.float64), faces=c.F, uvs=self.uvs32.astype(np.float64), face_mat=self.face_mat,
                              materials=self.materials)


_CASE = None


def pbr_case():
    global _CASE
    if _CASE is None:
        _CASE = PbrCase()
    return _CASE


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pc = PbrCase()
    print(f"{N_QUERIES} queries, {int(pc.on0.sum())} on material 0, {int(pc.border.sum())} of them near a texel border: "
          f"{pc.border.sum() / pc.on0.sum():.4f} (cap {BORDER_CAP}); none on material 1: {not pc.border[~pc.on0].any()}")
