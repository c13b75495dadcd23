"""The camera rig of the reference's rendering/blender_render_multiview.py as float64 matrices.

The mesh is rotated 90 degrees about x (OBJ y-up to Blender z-up), centred on the centre of its bounding box and scaled by
1 / (largest dimension / 2 * 1.03) (:43-52); the camera sits at distance 3 from the origin, looks at it with z up and has a 45 mm
lens on a 36 mm sensor (:92-104); there are eight views (azimuth, 45 degrees), azimuth 0, 45, ..., 315 (:93-95).  The light of
the rasteriser is overhead: +z after the rotation."""
import math

import numpy as np

DISTANCE = 3.0
FOCAL_MM, SENSOR_MM = 45.0, 36.0
VIEW_ANGLES = tuple((float(a), 45.0) for a in range(0, 360, 45))
ENLARGE = 1.03
NEAR = 0.1
ROT_X90 = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])       # (x, y, z) -> (x, -z, y)


class View:
    """matrix: float64 [4, 4], clip = matrix @ (x, y, z, 1) for a vertex as stored (only the x, y and w rows matter);
    light: unit vector towards the light in the space of the stored vertices; near: vertices with w <= near are flagged."""

    def __init__(self, matrix, light=(0.0, 0.0, 1.0), near=NEAR):
        self.matrix = np.asarray(matrix, dtype=np.float64).reshape(4, 4)
        light = np.asarray(light, dtype=np.float64).reshape(3)
        self.light = light / np.linalg.norm(light)
        self.near = float(near)


def camera_position(azimuth, elevation, d=DISTANCE):
    """blender_render_multiview.py:98-100, in degrees."""
    phi = azimuth / 180 * math.pi
    theta = elevation / 180 * math.pi
    return np.array([d * math.sin(theta) * math.cos(phi), d * math.sin(theta) * math.sin(phi), d * math.cos(theta)])


def normalization_matrix(vmin, vmax):
    """4 x 4: rotate 90 degrees about x, move the centre of the rotated bounding box to the origin, scale by
    1 / (largest dimension / 2 * 1.03)."""
    vmin, vmax = np.asarray(vmin, dtype=np.float64), np.asarray(vmax, dtype=np.float64)
    corners = np.array([[x, y, z] for x in (vmin[0], vmax[0]) for y in (vmin[1], vmax[1]) for z in (vmin[2], vmax[2])]) @ ROT_X90.T
    lo, hi = corners.min(0), corners.max(0)
    size = float((hi - lo).max()) / 2 * ENLARGE
    if not size > 0:
        size = 1.0                                           # a single point: leave the scale alone
    m = np.eye(4)
    m[:3, :3] = ROT_X90 / size
    m[:3, 3] = -(lo + hi) / 2 / size
    return m


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """(right, up, forward): the orthonormal camera axes of a camera at `eye` that looks at `target`."""
    eye = np.asarray(eye, dtype=np.float64)
    f = np.asarray(target, dtype=np.float64) - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, dtype=np.float64))
    r = r / np.linalg.norm(r)
    return r, np.cross(r, f), f


def view_projection(eye, resolution, focal=FOCAL_MM, sensor=SENSOR_MM):
    """World to clip for a pinhole camera at `eye` looking at the origin.  The sensor width spans the larger image side (Blender's
    sensor fit AUTO).  Row 3 gives w = the distance along the view direction; row 2 repeats it (the rasteriser reads no z)."""
    W, H = int(resolution[0]), int(resolution[1])
    r, u, f = look_at(eye)
    eye = np.asarray(eye, dtype=np.float64)
    s = 2.0 * focal / sensor * max(W, H)
    m = np.zeros((4, 4))
    m[0, :3], m[0, 3] = r * (s / W), -np.dot(r, eye) * (s / W)
    m[1, :3], m[1, 3] = u * (s / H), -np.dot(u, eye) * (s / H)
    m[3, :3], m[3, 3] = f, -np.dot(f, eye)
    m[2] = m[3]
    return m


def standard_views(vmin, vmax, resolution=(512, 512)):
    """The eight views of the rig for a mesh with this bounding box: object-to-clip matrices and the overhead light in object space."""
    model = normalization_matrix(vmin, vmax)
    light = ROT_X90.T @ np.array([0.0, 0.0, 1.0])            # +z after the rotation = +y of the stored mesh
    return [View(view_projection(camera_position(a, e), resolution) @ model, light, NEAR) for a, e in VIEW_ANGLES]
