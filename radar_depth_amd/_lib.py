"""ctypes binding of libradardepth_hip.so (the C ABI declared in include/radar_depth_hip.h).

The product path has NO fallback: if the library is missing or a call fails this raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# (RD_LIB_PATH: another build of the same ABI -- A/B runs of two kernel versions in one GPU job, tools/ab_lib.sh)
LIB_PATH = os.environ.get("RD_LIB_PATH") or os.path.join(HERE, "lib", "libradardepth_hip.so")

RD_MAX_TAPS = 25
RD_MAX_PHASES = 4
ACT_NONE, ACT_RELU, ACT_LEAKY02 = 0, 1, 2
# argument-check codes of the radar_filtered entry points (include/radar_depth_hip.h)
RD_ERADAR_NULL, RD_ERADAR_RANGE, RD_ERADAR_NRADAR, RD_ERADAR_NLIDAR, RD_ERADAR_FEWLIDAR, RD_ERADAR_CROP = -10, -11, -12, -13, -14, -15
# ... and of the lidar sparsifiers
RD_ESPARSE_NULL, RD_ESPARSE_RANGE, RD_ESPARSE_PIXELS, RD_ESPARSE_STRIDE, RD_ESPARSE_SAMPLES, RD_ESPARSE_MAXDEPTH = -20, -21, -22, -23, -24, -25
RD_ESPARSE_OVERLAP = -26
# ... and of the comparison-row renderer
RD_EVIS_NULL, RD_EVIS_RANGE, RD_EVIS_PLANES, RD_EVIS_STRIDE, RD_EVIS_PITCH, RD_EVIS_NAN, RD_EVIS_OVERLAP = -27, -28, -29, -30, -31, -32, -33
# ... and of the BerHu loss
RD_EBERHU_NULL, RD_EBERHU_RANGE, RD_EBERHU_THRESH, RD_EBERHU_ALIGN = -34, -35, -36, -37
# ... and of the distance-interval metrics
RD_EMDIST_NULL, RD_EMDIST_RANGE, RD_EMDIST_ALIGN, RD_EMDIST_EDGES, RD_EMDIST_FRAMES = -38, -39, -40, -41, -42
RD_MDIST_MAX_INTERVALS = 16
# ... and of the PnP-Depth kernels (csrc/pnp.hip)
RD_EPNP_NULL, RD_EPNP_RANGE, RD_EPNP_STRIDE, RD_EPNP_ACT, RD_EPNP_DTYPE, RD_EPNP_OVERLAP = -43, -44, -45, -46, -47, -48


class RdPhase(C.Structure):
    _fields_ = [("n_taps", C.c_int32), ("out_off_h", C.c_int32), ("out_off_w", C.c_int32),
                ("lh", C.c_int32), ("lw", C.c_int32),
                ("dh_min", C.c_int32), ("dh_max", C.c_int32), ("dw_min", C.c_int32), ("dw_max", C.c_int32),
                ("tile_begin", C.c_int32),
                ("dh", C.c_int8 * RD_MAX_TAPS), ("dw", C.c_int8 * RD_MAX_TAPS), ("widx", C.c_int16 * RD_MAX_TAPS)]


class RdConvDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Cin", C.c_int32), ("ldi", C.c_int32),
                ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32), ("ldo", C.c_int32),
                ("in_stride", C.c_int32), ("out_stride", C.c_int32), ("n_phases", C.c_int32),
                ("phase", RdPhase * RD_MAX_PHASES)]


class RdReduceJob(C.Structure):
    _fields_ = [("slabs", C.c_void_p), ("tmp", C.c_void_p), ("grad", C.c_void_p), ("E", C.c_int64),
                ("n_splits", C.c_int32), ("J", C.c_int32), ("S", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
                ("O", C.c_int32), ("I", C.c_int32), ("co_off", C.c_int32), ("accumulate", C.c_int32),
                ("first_block1", C.c_int32), ("n_blocks1", C.c_int32), ("first_block2", C.c_int32), ("n_blocks2", C.c_int32),
                ("pad_", C.c_int32)]


class RdStageTrainFrame(C.Structure):
    _fields_ = [("rot", C.c_double * 6), ("scale", C.c_double), ("factor", C.c_float * 3), ("order", C.c_int32 * 3),
                ("h_start", C.c_int32), ("w_start", C.c_int32), ("flip", C.c_int32), ("pad_", C.c_int32)]


class RadarDepthHipError(RuntimeError):
    pass


_lib = None


def lib():
    """Load the shared library once; fail loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RadarDepthHipError(
                "libradardepth_hip.so not built (%s). Run `python -m radar_depth_amd.build`; "
                "there is no CPU fallback for the HIP path." % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.rd_last_error.restype = C.c_char_p
        for name in ("rd_wgrad_workspace_floats", "rd_stem_wgrad_workspace_floats", "rd_smooth_workspace_floats",
                     "rd_head_conv_bwd_workspace_floats", "rd_gconv_workspace_floats", "rd_wgrad_bf16_workspace_floats",
                     "rd_wgrad_split_workspace_floats", "rd_stage_train_workspace_bytes", "rd_depth_metrics_frames_workspace_floats",
                     "rd_lidar_sparsify_workspace_bytes", "rd_render_workspace_bytes", "rd_berhu_workspace_floats",
                     "rd_depth_metrics_multidist_workspace_floats"):
            if hasattr(_lib, name):
                getattr(_lib, name).restype = C.c_int64
        # on-device metric meters (csrc/loss_opt.hip): full prototypes, so that None / plain ints marshal as the C side expects
        vp = C.c_void_p
        for name, args in (("rd_masked_l1_sums_metrics", [vp, vp, C.c_int64, vp, vp, vp, vp]),
                           ("rd_masked_l2_sums_metrics", [vp, vp, C.c_int64, vp, vp, vp, vp]),
                           # MaskedBerHuLoss (thresh travels as a double)
                           ("rd_berhu_workspace_floats", [C.c_int64]),
                           ("rd_masked_berhu_sums", [vp, vp, C.c_int64, C.c_double, vp, vp, vp]),
                           ("rd_masked_berhu_sums_metrics", [vp, vp, C.c_int64, C.c_double, vp, vp, vp, vp]),
                           ("rd_masked_berhu_bwd", [vp, vp, C.c_int64, vp, vp, vp, C.c_int32, vp]),
                           ("rd_depth_metrics_frames_workspace_floats", [C.c_int32, C.c_int64]),
                           ("rd_depth_metrics_frames", [vp, vp, C.c_int32, C.c_int64, vp, vp, vp]),
                           ("rd_meter_update", [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp]),
                           # the distance-interval metrics (csrc/metrics_multidist.hip)
                           ("rd_depth_metrics_multidist_workspace_floats", [C.c_int32, C.c_int64, C.c_int32]),
                           ("rd_depth_metrics_multidist", [vp, vp, C.c_int32, C.c_int64, vp, C.c_int32, vp, vp, vp]),
                           ("rd_meter_update_multidist", [vp, C.c_int32, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp]),
                           # the PnP-Depth kernels (csrc/pnp.hip)
                           ("rd_act_gate_t", [C.c_int32, vp, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.c_int64, C.c_int32, C.c_int32, vp]),
                           ("rd_pnp_update", [vp, C.c_int32, vp, C.c_int32, C.c_int64, C.c_int32, vp, vp]),
                           # the radar_filtered sparsifier (csrc/radar_filter.hip)
                           ("rd_radar_filter_points", [vp] * 6 + [C.c_int32] * 3 + [vp] * 5),
                           ("rd_radar_index_map", [vp, vp] + [C.c_int32] * 4 + [vp, vp]),
                           ("rd_stage_index_filter_val", [vp] * 3 + [C.c_int32] * 9 + [vp] * 3),
                           ("rd_stage_index_filter_train", [vp] * 3 + [C.c_int32] * 6 + [vp] * 3 + [C.c_int32] + [vp] * 3),
                           # the lidar sparsifiers (csrc/lidar_sparsify.hip)
                           ("rd_lidar_sparsify_workspace_bytes", [C.c_int32] * 3),
                           ("rd_lidar_radar_sparsify", [vp, C.c_int64, vp, C.c_int64] + [C.c_int32] * 3 + [vp, vp, C.c_int64, vp]),
                           ("rd_uniform_sparsify", [vp, C.c_int64] + [C.c_int32] * 3 + [C.c_int64, C.c_double, vp, C.c_uint64, C.c_uint64, vp, vp,
                                                                                      C.c_int64, vp, vp]),
                           # the comparison rows (csrc/visualize.hip)
                           ("rd_render_workspace_bytes", [C.c_int32]),
                           ("rd_render_rows", [vp, C.c_int64, vp, vp] + [C.c_int32] * 4 + [vp] * 4 + [C.c_int64, C.c_int64, vp])):
            if hasattr(_lib, name):
                getattr(_lib, name).argtypes = args
    return _lib


def check(rc, what=""):
    if rc != 0:
        raise RadarDepthHipError("%s failed (%d): %s" % (what, rc, lib().rd_last_error().decode()))


def ptr(t):
    """Device (or host) pointer of a torch tensor / None as c_void_p."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
