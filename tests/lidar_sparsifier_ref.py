"""numpy-only restatement of the reference's lidar sparsifiers (dataset/dense_to_sparse.py behind get_sparse_depth,
dataset/nuscenes_dataset_torch_new.py:200-216) with the tie rule written out: candidates of a radar pixel are ordered by (integer
squared pixel distance, row-major linear index) with a STABLE sort, where the reference's argsort of float distances is not stable.
tests/golden/make_golden_lidar_sparsifiers.py asserts that this file reproduces the reference's own code bit for bit on every golden
case (all of them free of ties between a radar pixel's second and third neighbour), so that the GPU tests can build further cases
from it alone.  Also here: Philox4x32-10 and the device generator's uniform numbers as include/radar_depth_hip.h defines them.
Nothing is shared with radar_depth_amd/dataset/dense_to_sparse.py on purpose."""
import numpy as np

import staging_train_ref as R


# ------------------------------------------------------------------------------------------------ lidar_radar
def _sorted_candidates(lidar, radar):
    """Per radar pixel (row-major order) the lidar pixels' linear indices sorted by (d^2, index), and the sorted d^2."""
    h, w = lidar.shape
    ry, rx = np.nonzero(radar > 0)
    lin = np.flatnonzero((lidar > 0).reshape(-1)).astype(np.int64)                # ascending: a stable sort keeps the lower index first
    ly, lx = lin // w, lin % w
    d2 = (ry[:, None] - ly[None, :]) ** 2 + (rx[:, None] - lx[None, :]) ** 2
    order = np.argsort(d2, axis=-1, kind="stable")
    return lin[order] if lin.size else np.zeros((len(ry), 0), np.int64), np.take_along_axis(d2, order, axis=-1)


def lidar_radar_mask(lidar, radar):
    """bool [h,w]: the union over the radar pixels of each one's two first candidates (all of them when there are fewer)."""
    lidar, radar = np.asarray(lidar), np.asarray(radar)
    cand, _ = _sorted_candidates(lidar, radar)
    mask = np.zeros(lidar.size, bool)
    mask[cand[:, :2].reshape(-1)] = True
    return mask.reshape(lidar.shape)


def n_tied(lidar, radar):
    """How many radar pixels have their second and third nearest lidar pixels at the same distance: where the reference's unstable
    argsort may choose otherwise."""
    _, d2 = _sorted_candidates(np.asarray(lidar), np.asarray(radar))
    return int((d2[:, 1] == d2[:, 2]).sum()) if d2.shape[1] >= 3 else 0


def lidar_radar_sparse(lidar, radar):
    """float32 [h,w]: lidar where the mask is set."""
    lidar = np.asarray(lidar, np.float32)
    return np.where(lidar_radar_mask(lidar, radar), lidar, np.float32(0))


# ------------------------------------------------------------------------------------------------ uniform
def uniform_mask(depth, num_samples, max_depth, draws):
    """bool, depth's shape.  The comparison with max_depth is torch's: the Python float rounded to fp32."""
    depth = np.asarray(depth, np.float32)
    keep = depth > 0
    if not np.isinf(max_depth):
        keep &= depth <= np.float32(max_depth)
    n_keep = int(np.count_nonzero(keep))
    if n_keep == 0:
        return keep
    prob = float(num_samples) / n_keep
    return keep & (np.asarray(draws, np.float64).reshape(depth.shape) < prob)


def uniform_sparse(depth, num_samples, max_depth, draws):
    depth = np.asarray(depth, np.float32)
    return np.where(uniform_mask(depth, num_samples, max_depth, draws), depth, np.float32(0))


# ------------------------------------------------------------------------------------------------ Philox4x32-10
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints.  Returns the four output words as uint64 arrays < 2^32."""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                       # 32 x 32 -> 64 bits: no overflow
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c


def philox_uniform(seed, frame, n):
    """float64 [n]: the device generator's numbers for the n pixels of frame number ``frame`` under ``seed``."""
    seed, frame = int(seed), int(frame) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((np.arange(n, dtype=np.uint64), frame & MASK32, frame >> 32, 0), (seed & MASK32, seed >> 32))
    return ((x[0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (x[1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def uniform_sparse_philox(depth, num_samples, max_depth, seed, offset):
    """depth [B,1,h,w] -> the sparse depth with the device generator, frame b numbered offset + b."""
    depth = np.asarray(depth, np.float32)
    return np.stack([uniform_sparse(depth[b], num_samples, max_depth, philox_uniform(seed, offset + b, depth[b].size)) for b in range(len(depth))])


# ------------------------------------------------------------------------------------------------ staged batches
def stage_val(image, lidar_i16, radar_i16, crop_size):
    """transform_val up to the sparsifier: (rgb [B,3,th,tw], lidar [B,1,th,tw], radar [B,1,th,tw]), the radar map not clamped."""
    B, H0, W0 = lidar_i16.shape
    th, tw = crop_size
    i0, j0 = int(round((H0 - th) / 2.)), int(round((W0 - tw) / 2.))
    win = (slice(None), slice(i0, i0 + th), slice(j0, j0 + tw))
    rgb = (image[win].astype(np.float32) / 255.).astype(np.float32).transpose(0, 3, 1, 2)
    return rgb, (lidar_i16[win] / 256.).astype(np.float32)[:, None], (radar_i16[win] / 256.).astype(np.float32)[:, None]


def stage_train(image, lidar_i16, radar_i16, p, crop_size):
    inputs, labels = R.transform_train_batch(image, lidar_i16, radar_i16, p, crop_size, np.inf)
    return inputs[:, :3], labels, inputs[:, 3:4]


def staged(mode, image, lidar_i16, radar_i16, p, crop_size, sparsifier, num_samples=0, max_depth=np.inf, draws=None):
    """(inputs [B,4,h,w], labels [B,1,h,w], the plane before the sparsifier [B,1,h,w]) of transform_val / transform_train with
    sparsifier lidar_radar or uniform (draws [B,1,h,w])."""
    rgb, lidar, radar = stage_val(image, lidar_i16, radar_i16, crop_size) if mode == "val" else stage_train(image, lidar_i16, radar_i16, p, crop_size)
    if sparsifier == "lidar_radar":
        plane = np.stack([lidar_radar_sparse(lidar[b, 0], radar[b, 0])[None] for b in range(len(lidar))])
    else:
        plane = np.stack([uniform_sparse(lidar[b], num_samples, max_depth, draws[b]) for b in range(len(lidar))])
    return np.concatenate((rgb, plane), 1).astype(np.float32), lidar, radar
