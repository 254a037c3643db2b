"""Host-side mirror of the reference's input staging (dataset/nuscenes_dataset_torch_new.py), GPU-backed."""
from .staging import (center_crop_params, draw_train_params, prepare_train_params, stage_train_batch,  # noqa: F401
                      stage_val_batch)
