"""Host-side mirror of the reference's input staging (dataset/nuscenes_dataset_torch_new.py), GPU-backed."""
from .dense_to_sparse import (LidarRadarSampling, UniformSampling, get_sparse_depth, lidar_radar_sparse_depth,  # noqa: F401
                              uniform_sparse_depth)
from .staging import (RadarFilter, center_crop_params, draw_train_params, filter_radar_points, prepare_train_params,  # noqa: F401
                      stage_train_batch, stage_val_batch)
