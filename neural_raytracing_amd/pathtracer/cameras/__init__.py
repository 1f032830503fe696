from .cameras import (Camera, DTUCamera, FoVPerspectiveCameras, NeRFCamera,  # noqa: F401
                      NeRFMMCamera, NeRVCamera, OpenGLPerspectiveCameras, look_at_rotation,
                      look_at_view_transform)
