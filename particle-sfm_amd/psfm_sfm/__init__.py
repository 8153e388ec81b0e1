from .convert import (read_model_arrays, save_depth_pose, sparse_depth_device, sparse_depth_host,  # noqa: F401
                      write_depth_pose_from_colmap_format)
