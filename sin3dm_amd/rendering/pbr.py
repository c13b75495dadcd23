"""PBR materials for the rasteriser: the MTL's PBR entries read beside data/obj_io.load_obj, the material table of
s3d_pbr_shade, and the three-light rig of the reference's rendering/blender_render_pbr.py as directional lights.

A material here is the dict of obj_io.load_obj ("Kd", "image") with, when present, "metallic_image" / "roughness_image" (uint8
[H, W], or [H, W, C] whose first channel is read) and "normal_image" (uint8 [H, W, 3]), all with row 0 on top, and the scalars
"Pm" / "Pr".  Absent maps fall back to the scalars; absent scalars to metallic 0 and roughness 0.5.

RIG_INTENSITY.  The reference's key / fill / rim area lights have energies 1 : 0.5 : 0.1 (blender_render_pbr.py:143-151).  As
directional lights of this light model a white Lambert surface (metallic 0, roughness 1, no Fresnel loss) that faced all three
squarely would show ambient + intensity * (1 + 0.5 + 0.1); with _lib.RENDER_PBR_AMBIENT = 0.1 and RIG_INTENSITY = 0.5 that is
0.9: a white sphere does not clip."""
from __future__ import annotations

import os
import warnings

import numpy as np

from .. import _lib
from . import camera

RIG_INTENSITY = _lib.RENDER_RIG_INTENSITY
RIG_RATIOS = (1.0, 0.5, 0.1)                                  # key : fill : rim
PBR_KEYS = {"map_Pm": "map_Pm", "map_Pr": "map_Pr", "map_Bump": "map_Bump", "map_bump": "map_Bump", "bump": "map_Bump", "norm": "map_Bump"}
DEFAULT_METALLIC, DEFAULT_ROUGHNESS = 0.0, 0.5


def three_light_rig(radius=2.0, height=10.0, intensity=RIG_INTENSITY):
    """float64 [3, 4]: unit direction towards the light and intensity of the key, fill and rim lights.  The reference places area
    lights at (radius, 0, height), (0, radius, 0.6 height) and (0, -radius, height) around the normalised, z-up mesh
    (blender_render_pbr.py:138-155); here each is a directional light from the origin towards that point, turned back into the
    axes of the stored (y-up) mesh."""
    pos = np.array([[radius, 0.0, height], [0.0, radius, 0.6 * height], [0.0, -radius, height]], dtype=np.float64)
    if not np.all(np.linalg.norm(pos, axis=1) > 0):
        raise ValueError(f"three_light_rig: radius {radius}, height {height}: a light at the origin has no direction")
    d = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    d = d @ camera.ROT_X90                                    # rows: ROT_X90.T @ direction
    return np.concatenate([d, float(intensity) * np.asarray(RIG_RATIOS)[:, None]], 1)


def parse_pbr_mtl(text):
    """{material name: {"map_Pm", "map_Pr", "map_Bump": file name, "Pm", "Pr": float}} with only the entries the text has.
    map_Bump, map_bump, bump and norm all name the normal map; options (-bm 1.0, -s ...) come before the file name."""
    mats, cur = {}, None
    for line in text.splitlines():
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        key = tok[0]
        if key == "newmtl":
            cur = mats.setdefault(" ".join(tok[1:]), {})
        elif cur is None or len(tok) < 2:
            continue
        elif key in PBR_KEYS:
            cur[PBR_KEYS[key]] = tok[-1]
        elif key in ("Pm", "Pr"):
            try:
                cur[key] = float(tok[1])
            except ValueError:
                warnings.warn(f"{key} {tok[1]!r} is not a number; the default is used")
    return mats


def _read_map(path, channels):
    """uint8 [H, W] (channels 1) or [H, W, 3], or None with a warning when PIL is missing or cannot read the file."""
    try:
        from PIL import Image
        with Image.open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert("L" if channels == 1 else "RGB"), dtype=np.uint8))
    except Exception as e:                                # noqa: BLE001 - whatever the decoder raises means "unreadable"
        warnings.warn(f"PBR map {path!r} cannot be read ({type(e).__name__}: {e}); the material falls back to its factor")
        return None


def load_pbr_maps(obj_path, materials):
    """The PBR entries of the MTL libraries of `obj_path` added to `materials`, the [(name, dict)] list of obj_io.load_obj (whose
    return value stays what it is): "metallic_image", "roughness_image", "normal_image" (None when absent or unreadable) and
    "Pm" / "Pr" where the MTL has them.  Returns the same list."""
    base = os.path.dirname(os.path.abspath(obj_path))
    library = {}
    with open(obj_path, errors="replace") as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if tok and tok[0] == "mtllib":
                p = os.path.join(base, " ".join(tok[1:]))
                if os.path.exists(p):
                    with open(p, errors="replace") as mh:
                        library.update(parse_pbr_mtl(mh.read()))
    for name, m in materials:
        extra = library.get(name, {})
        for key, field, ch in (("map_Pm", "metallic_image", 1), ("map_Pr", "roughness_image", 1), ("map_Bump", "normal_image", 3)):
            m[field] = _read_map(os.path.join(base, extra[key]), ch) if extra.get(key) else None
        for key in ("Pm", "Pr"):
            if key in extra:
                m[key] = extra[key]
    return materials


def has_pbr_info(materials):
    """{"albedo", "metallic", "roughness", "normal": bool}: whether some material carries that map or factor."""
    return {"albedo": any(m.get("image") is not None for m in materials),
            "metallic": any(m.get("metallic_image") is not None or "Pm" in m for m in materials),
            "roughness": any(m.get("roughness_image") is not None or "Pr" in m for m in materials),
            "normal": any(m.get("normal_image") is not None for m in materials)}


def pack_pbr_materials(materials, device):
    """(table int64 [M, 4, 3] = {byte offset, W, H} of the albedo / metallic / roughness / normal map, W = 0: absent; factors
    float32 [M, 5] = Kd, metallic, roughness — both NumPy, they are host arguments of s3d_pbr_shade —; images uint8 on
    `device`; image_bytes)."""
    import torch
    table = np.zeros((len(materials), 4, 3), dtype=np.int64)
    factors = np.zeros((len(materials), 5), dtype=np.float32)
    blobs, off = [], 0
    for i, m in enumerate(materials):
        factors[i, :3] = [float(x) for x in m.get("Kd", (1.0, 1.0, 1.0))]
        factors[i, 3] = float(m.get("Pm", DEFAULT_METALLIC))
        factors[i, 4] = float(m.get("Pr", DEFAULT_ROUGHNESS))
        for j, (field, ch) in enumerate((("image", 3), ("metallic_image", 1), ("roughness_image", 1), ("normal_image", 3))):
            img = m.get(field)
            if img is None:
                continue
            img = img if torch.is_tensor(img) else torch.from_numpy(np.array(img, dtype=np.uint8, order="C"))        # (a copy: PIL's is read-only)
            if img.dtype != torch.uint8 or img.dim() not in (2, 3) or (ch == 3 and (img.dim() != 3 or img.shape[2] < 3)):
                raise ValueError(f"pack_pbr_materials: material {i}, {field}: uint8 {'[H, W, 3]' if ch == 3 else '[H, W]'} expected, got "
                                 f"{img.dtype} {tuple(img.shape)}")
            img = img.to(device)
            img = img[..., :3] if ch == 3 else (img[..., 0] if img.dim() == 3 else img)
            img = img.contiguous()
            table[i, j] = [off, img.shape[1], img.shape[0]]
            blobs.append(img.reshape(-1))
            off += img.numel()
    images = torch.cat(blobs) if blobs else torch.zeros(1, device=device, dtype=torch.uint8)
    return table, factors, images.contiguous(), off
