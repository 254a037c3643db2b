"""The lidar sparsifiers on the GPU (csrc/lidar_sparsify.hip through dataset.lidar_radar_sparse_depth / uniform_sparse_depth and the
classes of dataset.dense_to_sparse) against the vectors of the reference's own code (tests/golden/lidar_sparsifiers.npz, every frame free
of ties) and, for what the reference cannot define (ties, the device generator), against the numpy restatement the generator pinned to
it (tests/lidar_sparsifier_ref.py).  Every decision is integer work or an IEEE float64 comparison, so every comparison is
np.array_equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_sparsifier_ref as S  # noqa: E402
from lidar_sparsifier_cases import G, LR_NAMES, PKEYS, STAGED, UN_NAMES, staged, tie_frame  # noqa: E402

pytestmark = pytest.mark.gpu
G_VAL = np.load(os.path.join(os.path.dirname(__file__), "golden", "staging.npz"))
G_TRAIN = np.load(os.path.join(os.path.dirname(__file__), "golden", "staging_train.npz"))


def gpu(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def planes(a):
    """[h,w] or [B,h,w] -> a [B,1,h,w] GPU tensor."""
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a.reshape((-1, 1) + a.shape[-2:]))).cuda()


def by_shape():
    out = {}
    for n in LR_NAMES:
        out.setdefault(G[n + "_lidar"].shape, []).append(n)
    return out


# ------------------------------------------------------------------------------------------------ lidar_radar
@pytest.mark.parametrize("name", LR_NAMES)
def test_lidar_radar_matches_reference_vectors(name):
    from radar_depth_amd.dataset import lidar_radar_sparse_depth
    assert int(G[name + "_n_tied"]) == 0
    got = lidar_radar_sparse_depth(planes(G[name + "_lidar"]), planes(G[name + "_radar"]))
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1) + G[name + "_lidar"].shape
    got = got.cpu().numpy()[0, 0]
    print("%s: %d pixels differ" % (name, (got != G[name + "_sparse"]).sum()))
    assert np.array_equal(got, G[name + "_sparse"])


@pytest.mark.parametrize("shape", sorted(by_shape()))
def test_lidar_radar_batch_of_17(shape):
    """All frames of one size in one batch, repeated to B = 17 (more than any per-launch chunk of frames), plain and with
    out = radar = inputs[:, 3:4] of a [B,4,h,w] tensor whose other planes must stay as they are."""
    from radar_depth_amd.dataset import lidar_radar_sparse_depth
    names = by_shape()[shape]
    names = [names[i % len(names)] for i in range(17)]
    lidar, radar, want = (np.stack([G[n + k] for n in names]) for k in ("_lidar", "_radar", "_sparse"))
    lt = planes(lidar)
    got = lidar_radar_sparse_depth(lt, planes(radar)).cpu().numpy()[:, 0]
    assert np.array_equal(got, want)
    inputs = torch.from_numpy(np.random.RandomState(1).rand(17, 4, *shape).astype(np.float32)).cuda()
    inputs[:, 3] = torch.from_numpy(radar).cuda()
    before = inputs.clone()
    ret = lidar_radar_sparse_depth(lt, inputs[:, 3:4], out=inputs[:, 3:4])
    assert ret.data_ptr() == inputs[:, 3:4].data_ptr()
    assert np.array_equal(inputs[:, 3].cpu().numpy(), want) and torch.equal(inputs[:, :3], before[:, :3])
    assert torch.equal(lt, planes(lidar))
    # the lidar plane as the neighbouring channel of the same tensor: interleaved with out, not overlapping it
    inputs[:, 3] = torch.from_numpy(radar).cuda()
    inputs[:, 2] = lt[:, 0]
    lidar_radar_sparse_depth(inputs[:, 2:3], inputs[:, 3:4], out=inputs[:, 3:4])
    assert np.array_equal(inputs[:, 3].cpu().numpy(), want) and torch.equal(inputs[:, 2:3], lt) and torch.equal(inputs[:, :2], before[:, :2])
    from radar_depth_amd._lib import RadarDepthHipError
    with pytest.raises(RadarDepthHipError, match="overlaps the lidar plane"):
        lidar_radar_sparse_depth(inputs[:, 2:3], inputs[:, 3:4], out=inputs[:, 2:3])
    assert torch.equal(inputs[:, 2:3], lt)                                        # rejected before anything was launched


def test_lidar_radar_equal_distances_go_to_the_lower_index():
    from radar_depth_amd.dataset import LidarRadarSampling, get_sparse_depth, lidar_radar_sparse_depth
    lidar, radar = tie_frame()
    want = S.lidar_radar_sparse(lidar, radar)
    assert (want != 0).sum() == 2 and want[7, 10] == lidar[7, 10] and want[10, 7] == lidar[10, 7]
    assert np.array_equal(lidar_radar_sparse_depth(planes(lidar), planes(radar)).cpu().numpy()[0, 0], want)
    f = LidarRadarSampling(100, 80.0)
    mask = f.dense_to_sparse(planes(lidar), planes(radar))
    assert mask.dtype == torch.bool and tuple(mask.shape) == (1, 1) + lidar.shape and np.array_equal(mask.cpu().numpy()[0, 0], want != 0)
    assert np.array_equal(get_sparse_depth(f, planes(lidar), planes(radar)).cpu().numpy()[0, 0], want)


def test_lidar_radar_larger_random_batch_with_ties_is_reproducible():
    from radar_depth_amd.dataset import lidar_radar_sparse_depth
    rng = np.random.RandomState(97161)
    B, h, w = 3, 97, 161
    lidar = (rng.uniform(1, 120, (B, h, w)) * (rng.rand(B, h, w) < 1500 / (h * w))).astype(np.float32)
    radar = (rng.uniform(1, 120, (B, h, w)) * (rng.rand(B, h, w) < 150 / (h * w))).astype(np.float32)
    want = np.stack([S.lidar_radar_sparse(lidar[b], radar[b]) for b in range(B)])
    print("lidar %s radar %s tied %s" % ((lidar > 0).sum((1, 2)), (radar > 0).sum((1, 2)), [S.n_tied(lidar[b], radar[b]) for b in range(B)]))
    assert sum(S.n_tied(lidar[b], radar[b]) for b in range(B)) > 0
    lt, rt = planes(lidar), planes(radar)
    one, two = lidar_radar_sparse_depth(lt, rt), lidar_radar_sparse_depth(lt, rt)
    assert np.array_equal(one.cpu().numpy()[:, 0], want) and torch.equal(one, two)


# ------------------------------------------------------------------------------------------------ uniform
@pytest.mark.parametrize("name", UN_NAMES)
def test_uniform_with_draws_matches_reference_vectors(name):
    from radar_depth_amd.dataset import UniformSampling, get_sparse_depth, uniform_sparse_depth
    depth, draws, ns, md = G[name + "_depth"], G[name + "_draws"], int(G[name + "_num_samples"]), float(G[name + "_max_depth"])
    dt, ut = planes(depth), planes(draws)
    got = uniform_sparse_depth(dt, ns, md, draws=ut).cpu().numpy()[0]
    print("%s: %d pixels differ" % (name, (got != G[name + "_sparse"]).sum()))
    assert np.array_equal(got, G[name + "_sparse"])
    f = UniformSampling(ns, md)
    mask = f.dense_to_sparse(dt, ut)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy()[0], S.uniform_mask(depth, ns, md, draws)) and f.offset == 0
    assert np.array_equal(get_sparse_depth(f, dt, draws=ut).cpu().numpy()[0], G[name + "_sparse"])


def test_uniform_batch_in_place():
    """The 33x47 cases that share num_samples = 100 as one strided batch, written over the depth plane itself."""
    from radar_depth_amd.dataset import uniform_sparse_depth
    names = ["un_empty", "un_inf", "un_empty", "un_inf", "un_inf"]
    depth, draws, want = (np.concatenate([G[n + k] for n in names]) for k in ("_depth", "_draws", "_sparse"))
    inputs = torch.zeros(5, 4, 33, 47, device="cuda")
    inputs[:, 3] = torch.from_numpy(depth).cuda()
    uniform_sparse_depth(inputs[:, 3:4], 100, draws=planes(draws), out=inputs[:, 3:4])
    assert np.array_equal(inputs[:, 3].cpu().numpy(), want) and not inputs[:, :3].any()


@pytest.mark.parametrize("offset", [0, 5, 2 ** 32 - 1])
def test_uniform_device_generator_matches_the_philox_restatement(offset):
    """Bit for bit, including a batch whose frame numbers carry into the second counter word."""
    from radar_depth_amd.dataset import uniform_sparse_depth
    rng = np.random.RandomState(4)
    depth = (rng.uniform(1, 120, (3, 1, 33, 47)) * (rng.rand(3, 1, 33, 47) < 0.4)).astype(np.float32)
    seed = 0x0123456789ABCDEF
    want = S.uniform_sparse_philox(depth, 200, 100.0, seed, offset)
    got = uniform_sparse_depth(planes(depth[:, 0]), 200, 100.0, seed=seed, offset=offset).cpu().numpy()
    print("offset %d: %d pixels differ, kept %s" % (offset, (got != want).sum(), (want != 0).sum((1, 2, 3))))
    assert np.array_equal(got, want) and (want != 0).any() and not np.array_equal(want[0], want[1])


def test_uniform_class_advances_its_offset():
    from radar_depth_amd.dataset import UniformSampling, get_sparse_depth
    rng = np.random.RandomState(6)
    depth = (rng.uniform(1, 120, (4, 1, 33, 47)) * (rng.rand(4, 1, 33, 47) < 0.4)).astype(np.float32)
    f = UniformSampling(150, 90.0, seed=77)
    dt = planes(depth[:, 0])
    first = f.dense_to_sparse(dt[:3])
    assert f.offset == 3
    second = get_sparse_depth(f, dt[3:])
    assert f.offset == 4
    want = S.uniform_sparse_philox(depth, 150, 90.0, 77, 0)
    assert np.array_equal(first.cpu().numpy(), want[:3] != 0) and np.array_equal(second.cpu().numpy(), want[3:])
    with pytest.raises(ValueError, match="exactly one of draws"):
        UniformSampling(150, 90.0).dense_to_sparse(dt)


# ------------------------------------------------------------------------------------------------ staged batches
@pytest.mark.parametrize("name,mode,sparsifier", STAGED)
def test_staging_then_sparsifier_matches_the_reference(name, mode, sparsifier):
    from radar_depth_amd.dataset import lidar_radar_sparse_depth, stage_train_batch, stage_val_batch, uniform_sparse_depth
    img, lidar, radar, p, crop, ns, md, draws, want_in, want_lb, before = staged(name)
    assert int(np.sum(G[name + "_n_tied"])) == 0
    t = gpu(img, lidar, radar)
    x, y = stage_val_batch(*t, crop, float("inf"), sparsifier="radar") if mode == "val" else \
        stage_train_batch(*t, p, crop, float("inf"), sparsifier="radar")
    assert np.array_equal(x[:, 3:4].cpu().numpy(), before)                       # the unclamped radar map the reference's sparsifier sees
    if sparsifier == "lidar_radar":
        lidar_radar_sparse_depth(y, x[:, 3:4], out=x[:, 3:4])
    else:
        uniform_sparse_depth(y, ns, md, draws=planes(draws[:, 0]), out=x[:, 3:4])
    x, y = x.cpu().numpy(), y.cpu().numpy()
    print("%s: %d input, %d label elements differ" % (name, (x != want_in).sum(), (y != want_lb).sum()))
    assert np.array_equal(x, want_in) and np.array_equal(y, want_lb)


def test_staging_defaults_still_match_the_staging_fixtures():
    from radar_depth_amd.dataset import lidar_radar_sparse_depth, stage_train_batch, stage_val_batch
    for name in ("a", "b", "c"):
        t = gpu(*(G_VAL[name + k] for k in ("_image", "_lidar", "_radar")))
        crop, md = tuple(int(v) for v in G_VAL[name + "_crop"]), float(G_VAL[name + "_max_depth"])
        got = stage_val_batch(*t, crop, md if np.isfinite(md) else -1.0)
        assert len(got) == 2 and np.array_equal(got[0].cpu().numpy(), G_VAL[name + "_inputs"]) and np.array_equal(got[1].cpu().numpy(), G_VAL[name + "_labels"])
    for name in ("six", "rag1"):
        t = gpu(*(G_TRAIN[name + k] for k in ("_image", "_lidar", "_radar")))
        p = {k: G_TRAIN["%s_p_%s" % (name, k)] for k in PKEYS}
        crop, md = tuple(int(v) for v in G_TRAIN[name + "_crop"]), float(G_TRAIN[name + "_max_depth"])
        got = stage_train_batch(*t, p, crop, md if np.isfinite(md) else -1.0)
        assert len(got) == 2 and np.array_equal(got[0].cpu().numpy(), G_TRAIN[name + "_inputs"]) and np.array_equal(got[1].cpu().numpy(), G_TRAIN[name + "_labels"])
        # and the sparsifier behind it leaves rgb and labels alone
        x, y = got[0].clone(), got[1].clone()
        lidar_radar_sparse_depth(y, x[:, 3:4], out=x[:, 3:4])
        want = np.stack([S.lidar_radar_sparse(G_TRAIN[name + "_labels"][b, 0], G_TRAIN[name + "_inputs"][b, 3]) for b in range(len(x))])
        assert np.array_equal(x[:, 3].cpu().numpy(), want) and torch.equal(x[:, :3], got[0][:, :3]) and torch.equal(y, got[1])
