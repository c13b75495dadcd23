"""Multi-view renders of meshes on the device: the reference's camera rig (camera.py), the tiled rasteriser
(rasterizer.py over s3d_render.hip) and the command line with the reference's flags (render_multiview.py)."""
from .camera import View, standard_views                      # noqa: F401
from .rasterizer import project, rasterize, render_views      # noqa: F401
