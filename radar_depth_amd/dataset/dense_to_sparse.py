"""The lidar sparsifiers on the GPU: the reference's ``dataset/dense_to_sparse.py`` (``UniformSampling``, ``LidarRadarSampling``) and
``get_sparse_depth`` (dataset/nuscenes_dataset_torch_new.py:200-216) for a whole staged batch.

Both work on the depth maps AFTER the transform, i.e. on what ``stage_val_batch`` / ``stage_train_batch`` return: ``labels`` is the lidar
depth and, staged with ``sparsifier="radar", max_depth=inf``, ``inputs[:, 3:4]`` is the unclamped radar depth the reference hands to
``get_sparse_depth``.  The sparsifier then overwrites that plane::

    inputs, labels = stage_train_batch(image, lidar, radar, params, crop_size)                  # sparsifier="radar", no clamp
    lidar_radar_sparse_depth(labels, inputs[:, 3:4], out=inputs[:, 3:4])                         # --sparsifier lidar_radar
    uniform_sparse_depth(labels, num_samples, max_depth, seed=seed, offset=frame0, out=inputs[:, 3:4])      # --sparsifier uniform

``lidar_radar``: equal pixel distances go to the lower row-major index (the reference's argsort is unstable; the two agree wherever a
radar pixel's second and third nearest lidar pixels are not equidistant).  ``uniform``: bit-identical to the reference with its own
draws (``draws=``), or a Philox4x32-10 stream on the device (``seed=``, ``offset=``; defined in include/radar_depth_hip.h).  Kernels:
csrc/lidar_sparsify.hip.  Nothing synchronises with the host and there is no CPU fallback."""
import numpy as np
import torch

from .._lib import check, current_stream, lib, ptr


def _planes(t, what, dtype=torch.float32):
    """[B,1,h,w] on the GPU, every frame contiguous, any batch stride -> (B, h, w, batch stride in elements)."""
    assert torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 4 and t.shape[1] == 1, "%s: %s [B,1,h,w] on the GPU" % (what, dtype)
    B, _, h, w = t.shape
    assert B >= 1 and h >= 1 and w >= 1, what + ": empty"
    assert (w == 1 or t.stride(3) == 1) and (h == 1 or t.stride(2) == w), what + ": every frame must be contiguous"
    return B, h, w, (t.stride(0) if B > 1 else h * w)


def _out_like(out, ref, what):
    if out is None:
        return torch.empty(ref.shape, dtype=torch.float32, device=ref.device)
    assert tuple(out.shape) == tuple(ref.shape) and out.device == ref.device, what + ": out has another shape or device"
    return out


def _workspace(L, B, h, w, dev):
    # (a geometry the library rejects gives a negative size here; the call that follows reports it)
    return torch.empty(max(int(L.rd_lidar_sparsify_workspace_bytes(B, h, w)), 16), dtype=torch.uint8, device=dev)


def lidar_radar_sparse_depth(lidar_depth, radar_depth, out=None):
    """``LidarRadarSampling`` + ``get_sparse_depth`` for a batch: the lidar depth at the two lidar pixels (``lidar_depth > 0``) nearest
    to every radar pixel (``radar_depth > 0``), zero elsewhere.  lidar_depth / radar_depth: fp32 [B,1,h,w] on the GPU, each frame
    contiguous, any batch stride (``inputs[:, 3:4]`` is taken as it is).  ``out``: such a view to write into; it may be ``radar_depth``
    itself (the radar pixels are collected before the plane is cleared); any other overlap with an input is an error.  Returns the
    sparse depth [B,1,h,w].
    Queued on the current stream; the point counts never reach the host."""
    B, h, w, ls = _planes(lidar_depth, "lidar_depth")
    assert _planes(radar_depth, "radar_depth")[:3] == (B, h, w) and radar_depth.device == lidar_depth.device, "radar_depth: another shape or device"
    out = _out_like(out, lidar_depth, "lidar_radar_sparse_depth")
    rs, os_ = _planes(radar_depth, "radar_depth")[3], _planes(out, "out")[3]
    L = lib()
    work = _workspace(L, B, h, w, lidar_depth.device)
    check(L.rd_lidar_radar_sparsify(ptr(lidar_depth), ls, ptr(radar_depth), rs, B, h, w, ptr(work), ptr(out), os_, current_stream()),
          "rd_lidar_radar_sparsify")
    return out


def _one_of(draws, seed):
    if (draws is None) == (seed is None):
        raise ValueError("uniform sparsifier: exactly one of draws (the reference's np.random.uniform(0, 1, depth.shape)) and seed (the "
                         "device generator) must be given")


def _uniform(depth, num_samples, max_depth, draws, seed, offset, out, mask):
    _one_of(draws, seed)
    B, h, w, ds = _planes(depth, "depth")
    out = _out_like(out, depth, "uniform_sparse_depth")
    os_ = _planes(out, "out")[3]
    if draws is not None:
        assert _planes(draws, "draws", torch.float64)[:3] == (B, h, w) and draws.device == depth.device, "draws: float64 [B,1,h,w] like depth"
        draws = draws.contiguous()
    if seed is not None:
        seed, offset = int(seed), int(offset)
        assert 0 <= seed < 1 << 64 and 0 <= offset and offset + B <= 1 << 64, "seed and frame numbers are unsigned 64-bit integers"
    L = lib()
    work = _workspace(L, B, h, w, depth.device)
    check(L.rd_uniform_sparsify(ptr(depth), ds, B, h, w, int(num_samples), float(max_depth), ptr(draws), seed or 0, offset if seed is not None else 0,
                                ptr(work), ptr(out), os_, ptr(mask), current_stream()), "rd_uniform_sparsify")
    return out


def uniform_sparse_depth(depth, num_samples, max_depth=float("inf"), draws=None, seed=None, offset=0, out=None):
    """``UniformSampling`` + ``get_sparse_depth`` for a batch: of the pixels with ``depth > 0`` (and ``depth <= max_depth``, compared in
    fp32 as torch does) each is kept with probability ``num_samples / n_keep`` of its frame.  depth: fp32 [B,1,h,w] on the GPU (each
    frame contiguous, any batch stride).  Exactly one of
      draws   float64 [B,1,h,w] on the GPU: the reference's ``np.random.uniform(0, 1, depth.shape)`` of every frame -> bit-identical to it
      seed    the device generator (Philox4x32-10, include/radar_depth_hip.h); ``offset`` is the global number of the batch's first
              frame, so that a stream of batches never reuses a frame's numbers
    must be given (``ValueError`` otherwise).  ``out``: a view to write into (it may be ``depth`` itself; any other overlap is an
    error).  Returns the sparse depth."""
    return _uniform(depth, num_samples, max_depth, draws, seed, offset, out, None)


class _Sampling:
    """What the two sparsifier objects share: the reference's constructor arguments kept as attributes, and its printed form
    ``<name>{ns=<num_samples>,md=<max_depth>}`` (main.py puts it into the name of the output directory)."""
    name = None

    def __init__(self, num_samples, max_depth=np.inf):
        self.num_samples, self.max_depth = num_samples, max_depth

    def __repr__(self):
        return "{}{{ns={:d},md={:f}}}".format(self.name, int(self.num_samples), float(self.max_depth))

    def dense_to_sparse(self, *planes):
        raise NotImplementedError("dense_to_sparse: UniformSampling and LidarRadarSampling have one")


class UniformSampling(_Sampling):
    """``--sparsifier uniform`` for a batch on the GPU.  With ``seed`` the device generator is used and the object numbers the frames
    it has seen (``offset``, advanced by B per call); without, every call needs the reference's ``draws``."""
    name = "uar"

    def __init__(self, num_samples, max_depth=np.inf, seed=None):
        super().__init__(num_samples, max_depth)
        self.seed, self.offset = seed, 0

    def _run(self, depth, draws, out):
        _one_of(draws, self.seed if draws is None else None)
        mask = torch.empty(depth.shape, dtype=torch.uint8, device=depth.device)
        generated = draws is None
        out = _uniform(depth, self.num_samples, self.max_depth, draws, self.seed if generated else None, self.offset, out, mask)
        if generated:
            self.offset += depth.shape[0]
        return out, mask.view(torch.bool)

    def dense_to_sparse(self, depth, draws=None):
        """bool [B,1,h,w]: the pixels kept."""
        return self._run(depth, draws, None)[1]


class LidarRadarSampling(_Sampling):
    """``--sparsifier lidar_radar`` for a batch on the GPU; ``num_samples`` and ``max_depth`` are accepted and unused, as in the
    reference."""
    name = "lidar_radar"

    def dense_to_sparse(self, lidar_depth, radar_depth):
        """bool [B,1,h,w]: the chosen lidar pixels (their depth is positive, so they are the non-zero pixels of the sparse depth)."""
        return lidar_radar_sparse_depth(lidar_depth, radar_depth) != 0


def get_sparse_depth(sparsifier_func, lidar_depth, radar_depth=None, out=None, **kw):
    """The reference's ``get_sparse_depth`` with the sparsifier object as an argument: the sparse depth [B,1,h,w] of ``lidar_depth``
    under a ``UniformSampling`` (``draws=`` may be passed along) or a ``LidarRadarSampling`` (needs ``radar_depth``)."""
    draws = kw.pop("draws", None)
    if kw:
        raise TypeError("get_sparse_depth: unexpected keyword %s" % sorted(kw))
    if isinstance(sparsifier_func, UniformSampling):
        return sparsifier_func._run(lidar_depth, draws, out)[0]
    if isinstance(sparsifier_func, LidarRadarSampling):
        assert radar_depth is not None
        return lidar_radar_sparse_depth(lidar_depth, radar_depth, out=out)
    raise ValueError("[Error] Invalid lidar sparsifier.")
