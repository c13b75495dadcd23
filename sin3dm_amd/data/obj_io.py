"""A Wavefront OBJ / MTL reader on NumPy alone (the reference loads through trimesh): triangles with per-corner uv and a
material per face."""
import os
import warnings

import numpy as np

DEFAULT_MATERIAL = {"Ka": (0.0, 0.0, 0.0), "Kd": (1.0, 1.0, 1.0), "Ks": (0.4, 0.4, 0.4), "Ns": 10.0, "map_Kd": None}


def parse_mtl(text):
    """{name: {"Ka", "Kd", "Ks": 3 floats, "Ns": float, "map_Kd": file name or None}} in file order."""
    mats, cur = {}, None
    for line in text.splitlines():
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        key = tok[0]
        if key == "newmtl":
            cur = mats.setdefault(" ".join(tok[1:]), dict(DEFAULT_MATERIAL))
        elif cur is None:
            continue
        elif key in ("Ka", "Kd", "Ks") and len(tok) >= 4:
            cur[key] = tuple(float(x) for x in tok[1:4])
        elif key == "Ns" and len(tok) >= 2:
            cur["Ns"] = float(tok[1])
        elif key == "map_Kd" and len(tok) >= 2:
            cur["map_Kd"] = tok[-1]                       # options (-s, -o ...) come before the file name
    return mats


def _read_image(path):
    """uint8 [H, W, 3], or None with a warning when PIL is missing or cannot read the file."""
    try:
        from PIL import Image
        with Image.open(path) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
    except Exception as e:                                # noqa: BLE001 - whatever the decoder raises means "unreadable"
        warnings.warn(f"map_Kd {path!r} cannot be read ({type(e).__name__}: {e}); the material falls back to its Kd")
        return None


def parse_obj(text, mtl_loader=None):
    """The mesh of an OBJ text: dict with
    verts [V, 3] float64, faces [F, 3] int64, uvs [F, 3, 2] float64 (0 where a corner has no vt), face_mat [F] int32,
    materials: list of (name, dict) in order of first use, n_degenerate: dropped faces (a repeated vertex index or zero area).
    Faces are `v`, `v/vt`, `v//vn` or `v/vt/vn`, indices from 1 or negative (from the end); polygons are fan-triangulated.
    mtl_loader(file name) -> MTL text, called for every mtllib line (None: materials keep the defaults)."""
    verts, vts, faces, fuv, fmat = [], [], [], [], []
    library, used, cur = {}, {}, None

    def mat_id(name):
        if name not in used:
            used[name] = len(used)
        return used[name]

    for line in text.splitlines():
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        key = tok[0]
        if key == "v":
            verts.append([float(x) for x in tok[1:4]])
        elif key == "vt":
            vts.append([float(tok[1]), float(tok[2]) if len(tok) > 2 else 0.0])
        elif key == "mtllib" and mtl_loader is not None:
            txt = mtl_loader(" ".join(tok[1:]))
            if txt is not None:
                library.update(parse_mtl(txt))
        elif key == "usemtl":
            cur = " ".join(tok[1:])
        elif key == "f":
            corners = []
            for c in tok[1:]:
                parts = c.split("/")
                vi = int(parts[0])
                vi = vi - 1 if vi > 0 else len(verts) + vi
                ti = None
                if len(parts) > 1 and parts[1]:
                    ti = int(parts[1])
                    ti = ti - 1 if ti > 0 else len(vts) + ti
                if not 0 <= vi < len(verts) or (ti is not None and not 0 <= ti < len(vts)):
                    raise ValueError(f"face index out of range in {line.strip()!r}")
                corners.append((vi, ti))
            m = mat_id(cur)
            for k in range(1, len(corners) - 1):
                tri = (corners[0], corners[k], corners[k + 1])
                faces.append([c[0] for c in tri])
                fuv.append([c[1] if c[1] is not None else -1 for c in tri])
                fmat.append(m)
    V = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    Fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ti = np.asarray(fuv, dtype=np.int64).reshape(-1, 3)
    vt = np.concatenate([np.asarray(vts, dtype=np.float64).reshape(-1, 2), np.zeros((1, 2))])      # index -1: uv 0
    uvs = vt[ti]
    fm = np.asarray(fmat, dtype=np.int32)
    if Fc.shape[0]:
        a, b, c = V[Fc[:, 0]], V[Fc[:, 1]], V[Fc[:, 2]]
        keep = (Fc[:, 0] != Fc[:, 1]) & (Fc[:, 1] != Fc[:, 2]) & (Fc[:, 0] != Fc[:, 2]) & (np.linalg.norm(np.cross(b - a, c - a), axis=1) > 0)
    else:
        keep = np.zeros(0, dtype=bool)
    materials = [(n if n is not None else "default", dict(library.get(n, DEFAULT_MATERIAL))) for n in used] or [("default", dict(DEFAULT_MATERIAL))]
    return {"verts": V, "faces": Fc[keep], "uvs": uvs[keep], "face_mat": fm[keep], "materials": materials, "n_degenerate": int((~keep).sum())}


def load_obj(path):
    """parse_obj of a file, its MTL libraries and images read from the same directory: every material gets "image" (uint8 [H, W, 3]
    or None).  A map_Kd that cannot be read falls back to Kd with a warning."""
    base = os.path.dirname(os.path.abspath(path))

    def loader(name):
        p = os.path.join(base, name)
        if not os.path.exists(p):
            warnings.warn(f"mtllib {name!r} not found beside {path}; default materials")
            return None
        with open(p, errors="replace") as fh:
            return fh.read()

    with open(path, errors="replace") as fh:
        mesh = parse_obj(fh.read(), loader)
    for _, m in mesh["materials"]:
        m["image"] = _read_image(os.path.join(base, m["map_Kd"])) if m.get("map_Kd") else None
    return mesh
