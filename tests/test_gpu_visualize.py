"""The comparison rows on the GPU (csrc/visualize.hip through radar_depth_amd.utils.merge_into_row, merge_into_row_with_gt,
colored_depthmap and ComparisonImage) against the vectors of the reference's own utils functions (tests/golden/visualize.npz) and, at
a size the fixture does not hold, against the numpy restatement the generator pinned to them (tests/visualize_ref.py).  Every value is
a table row chosen by float32 arithmetic that the kernel restates operation by operation, so every comparison is np.array_equal.
Neither matplotlib nor Pillow is imported here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visualize_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "visualize.npz"))
CASES = ("rgbd1", "rgb1", "rgb2", "ladder", "const", "edge")


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def render(name):
    """The case through the public functions the way main.py:662-677 slices: rgb and the sparse depth are views of one tensor."""
    from radar_depth_amd import utils
    inputs, target, pred = gpu(G[name + "_inputs"]), gpu(G[name + "_target"]), gpu(G[name + "_pred"])
    if inputs.shape[1] == 4:
        return utils.merge_into_row_with_gt(inputs[:, :3], inputs[:, 3:], target, pred)
    return utils.merge_into_row(inputs, target, pred)


@pytest.mark.parametrize("name", CASES)
def test_single_frames_match_reference_rows(name):
    want = G[name + "_rows"][0]
    got = render(name)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape       # [H, kW, 3]: the reference's shape for B = 1
    got = got.cpu().numpy()
    print("%s: %d of %d pixels differ" % (name, (got != want).any(axis=-1).sum(), want.shape[0] * want.shape[1]))
    assert np.array_equal(got, want)


def test_ladder_pixels_one_by_one():
    """The 510 boundary depths of the prediction panel: each takes exactly the reference's colour (a reciprocal or float64 shortcut
    changes more than a hundred of them)."""
    got = render("ladder").cpu().numpy()[:, 3 * 80:].reshape(-1, 3)[G["ladder_pos"]]
    want = G["ladder_rows"][0][:, 3 * 80:].reshape(-1, 3)[G["ladder_pos"]]
    print("ladder: %d of 510 boundary pixels differ" % (got != want).any(axis=-1).sum())
    assert np.array_equal(got, want)


def test_batch_of_channel_slices_every_frame_its_own_range():
    from radar_depth_amd import utils
    inputs, target, pred = gpu(G["batch_inputs"]), gpu(G["batch_target"]), gpu(G["batch_pred"])
    before = inputs.clone()
    got = utils.merge_into_row_with_gt(inputs[:, :3], inputs[:, 3:4], target, pred)
    assert tuple(got.shape) == (5, 33, 4 * 47, 3) and torch.equal(inputs, before)
    assert np.array_equal(got.cpu().numpy(), G["batch_rows"])
    rgb_rows = utils.merge_into_row(inputs[:, :3], target, pred).cpu().numpy()               # k = 3 from the same tensor
    assert np.array_equal(rgb_rows, V.merge_rows(G["batch_inputs"][:, :3], [G["batch_target"], G["batch_pred"]], G["table"]))


def test_colored_depthmap():
    from radar_depth_amd import utils
    depth, flat = gpu(G["cmap_depth"]), gpu(G["cmap_flat"])
    d_min, d_max = (float(v) for v in G["cmap_range"])
    got = utils.colored_depthmap(depth, d_min, d_max)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (33, 47, 3)
    assert np.array_equal(got.cpu().numpy(), G["cmap_img"])                                    # below, above, exactly on d_max
    assert np.array_equal(utils.colored_depthmap(depth).cpu().numpy(), G["cmap_img_own"])     # the plane's own range
    assert np.array_equal(utils.colored_depthmap(flat, 7.5, 7.5).cpu().numpy(), G["cmap_flat_img"])      # d_min == d_max: under / bad / over
    both = utils.colored_depthmap(torch.stack([depth, flat])[:, None])                        # [B,1,H,W]: every frame its own range
    assert tuple(both.shape) == (2, 33, 47, 3) and np.array_equal(both[0].cpu().numpy(), G["cmap_img_own"])
    assert np.array_equal(both[1].cpu().numpy(), V.colored_depthmap(G["cmap_flat"], G["table"]))


def test_canvas_rows_start_on_odd_bytes():
    """Three k = 3, W = 47 rows in one ComparisonImage: rows 1 and 2 start 13959 and 27918 bytes into the canvas."""
    from radar_depth_amd import utils
    names = ("rgb1", "edge", "rgb2")
    canvas = utils.ComparisonImage(3, 33, 47, 3)
    assert (canvas.row(1).data_ptr() - canvas.row(0).data_ptr()) % 4 == 3
    for i, name in enumerate(names):
        inputs, target, pred = gpu(G[name + "_inputs"]), gpu(G[name + "_target"]), gpu(G[name + "_pred"])
        ret = utils.merge_into_row(inputs, target, pred, out=canvas.row(i))
        assert ret.data_ptr() == canvas.row(i).data_ptr()
    want = np.vstack([G[name + "_rows"][0] for name in names])
    assert np.array_equal(canvas.numpy(), want)
    assert np.array_equal(utils.add_row(utils.add_row(render("rgb1"), render("edge")), render("rgb2")).cpu().numpy(), want)


@pytest.mark.parametrize("offset", (0, 1, 2, 3))
def test_out_inside_a_larger_buffer_leaves_guard_bytes(offset):
    """B = 5 rows rendered at a byte offset into a buffer with a wider pitch and a longer frame stride: the bytes before, after, in the
    pitch padding and between the frames keep their value."""
    from radar_depth_amd import utils
    inputs, target, pred = gpu(G["batch_inputs"]), gpu(G["batch_target"]), gpu(G["batch_pred"])
    B, H, L = 5, 33, 3 * 4 * 47
    pitch, lead = L + 7, 64 + offset
    frame = H * pitch + 5
    buf = torch.full((lead + B * frame + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf.as_strided((B, H, 4 * 47, 3), (frame, pitch, 3, 1), lead)
    utils.merge_into_row_with_gt(inputs[:, :3], inputs[:, 3:4], target, pred, out=out)
    assert np.array_equal(out.cpu().numpy(), G["batch_rows"])
    written = torch.zeros_like(buf, dtype=torch.bool)
    written.as_strided((B, H, L), (frame, pitch, 1), lead).fill_(True)
    assert int(written.sum()) == B * H * L and bool((buf[~written] == 0xA5).all())


def test_full_size_batch_against_the_restatement():
    """450x800, B = 2: several workgroups per frame feed the range atomics, 16-byte loads, dword stores."""
    from radar_depth_amd import utils
    rng = np.random.RandomState(5)
    inputs = rng.rand(2, 4, 450, 800).astype(np.float32)
    inputs[:, 3] = (rng.uniform(2, 100, (2, 450, 800)) * (rng.rand(2, 450, 800) < 0.02)).astype(np.float32)
    target = (rng.uniform(2, 118, (2, 1, 450, 800)) * (rng.rand(2, 1, 450, 800) < 0.3)).astype(np.float32)
    pred = rng.uniform(-1, 90, (2, 1, 450, 800)).astype(np.float32)
    pred[1] *= np.float32(0.01)
    target[1] *= np.float32(0.01)
    inputs[1, 3] *= np.float32(0.01)
    target[0, 0, 449, 799], pred[1, 0, 449, 799] = 119.5, -3.0                                # the extremes in the last pixel of a plane
    ti = gpu(inputs)
    got = utils.merge_into_row_with_gt(ti[:, :3], ti[:, 3:4], gpu(target), gpu(pred)).cpu().numpy()
    want = V.merge_rows(inputs[:, :3], [inputs[:, 3:4], target, pred], G["table"])
    print("450x800: %d of %d pixels differ" % ((got != want).any(axis=-1).sum(), want.size // 3))
    assert np.array_equal(got, want)


def test_repeated_calls_are_identical():
    first = render("rgbd1")
    for _ in range(5):
        assert torch.equal(render("rgbd1"), first)
    from radar_depth_amd import utils
    inputs, target, pred = gpu(G["batch_inputs"]), gpu(G["batch_target"]), gpu(G["batch_pred"])
    a = utils.merge_into_row_with_gt(inputs[:, :3], inputs[:, 3:4], target, pred)
    b = utils.merge_into_row_with_gt(inputs[:, :3], inputs[:, 3:4], target, pred)
    assert torch.equal(a, b)
