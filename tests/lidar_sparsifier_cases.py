"""What the host and the GPU tests of the lidar sparsifiers share: the fixture (tests/golden/lidar_sparsifiers.npz), the names of its
cases, the staged cases unpacked, and the hand-built frame of the tie rule."""
import os

import numpy as np

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "lidar_sparsifiers.npz"))
LR_NAMES = ["lr_l0", "lr_l1", "lr_l2", "lr_l63", "lr_l64", "lr_l65", "lr_norad", "lr_special", "lr_l300", "lr_special2"]
UN_NAMES = ["un_empty", "un_ns0", "un_all", "un_inf", "un_md", "un_big"]
STAGED = [("val_lr", "val", "lidar_radar"), ("tr_lr", "train", "lidar_radar"), ("val_un", "val", "uniform"), ("tr_un", "train", "uniform")]
PKEYS = ("scale", "angle", "flip", "h_start", "w_start", "factors", "order")


def tie_frame():
    """One radar pixel with four lidar pixels at distance 3 (and one at 5), every lidar pixel with a depth of its own."""
    lidar, radar = np.zeros((21, 25), np.float32), np.zeros((21, 25), np.float32)
    radar[10, 10] = 40.0
    for k, (y, x) in enumerate([(10, 13), (13, 10), (7, 10), (10, 7), (14, 13)]):
        lidar[y, x] = 10.0 + k
    return lidar, radar


def staged(name):
    p = {k: G["%s_p_%s" % (name, k)] for k in PKEYS} if name + "_p_scale" in G.files else None
    draws = G[name + "_draws"] if name + "_draws" in G.files else None
    return (G[name + "_image"], G[name + "_lidar"], G[name + "_radar"], p, tuple(int(v) for v in G[name + "_crop"]), int(G[name + "_num_samples"]),
            float(G[name + "_max_depth"]), draws, G[name + "_inputs"], G[name + "_labels"], G[name + "_plane_before"])
