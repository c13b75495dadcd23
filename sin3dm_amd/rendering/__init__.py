"""Multi-view renders of meshes on the device: the reference's camera rig (camera.py), the tiled rasteriser
(rasterizer.py over s3d_render.hip) and the command line with the reference's flags (render_multiview.py); smooth normals,
normal maps, the GGX light model and the material passes (s3d_render_pbr.hip, pbr.py, render_pbr.py)."""
from .camera import View, standard_views                      # noqa: F401
from .rasterizer import face_tangents, project, rasterize, render_views, vertex_normals      # noqa: F401
