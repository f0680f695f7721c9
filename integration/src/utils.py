"""Drop-in for /root/reference/src/utils.py (imported by infer.py:1, val.py)."""
from mvd_amd.utils import create_camera_matrix, create_output_dirs, load_image, log_debug  # noqa: F401
from mvd_amd.utils import orbit_cameras  # noqa: F401  (not in the reference: target poses for MVDPipeline.generate_views)
