"""Host-side mirror of the reference's input staging (dataset/nuscenes_dataset_torch_new.py), GPU-backed."""
from .staging import (RadarFilter, center_crop_params, draw_train_params, filter_radar_points, prepare_train_params,  # noqa: F401
                      stage_train_batch, stage_val_batch)
