from .convert import (colour_table, depth_display_device, depth_display_host, read_model_arrays, save_depth_pose,  # noqa: F401
                      sparse_depth_batches, sparse_depth_device, sparse_depth_host, write_depth_pose_from_colmap_format)
