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

# ... and of the KITTI devkit evaluation (csrc/kitti_eval.hip)
RD_EKITTI_NULL, RD_EKITTI_RANGE, RD_EKITTI_STRIDE, RD_EKITTI_ALIGN, RD_EKITTI_PITCH, RD_EKITTI_OVERLAP = -49, -50, -51, -52, -53, -54


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
# type characters of the library's prototype table (rd_abi_entry, include/radar_depth_hip.h)
_CTYPE = {"p": C.c_void_p, "s": C.c_char_p, "f": C.c_float, "d": C.c_double,
          "b": C.c_int8, "h": C.c_int16, "i": C.c_int32, "l": C.c_int64,
          "B": C.c_uint8, "H": C.c_uint16, "I": C.c_uint32, "L": C.c_uint64}


def lib():
    """Load the shared library once; fail loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RadarDepthHipError(
                "libradardepth_hip.so not built (%s). Run `python -m radar_depth_amd.build`; "
                "there is no CPU fallback for the HIP path." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        if not hasattr(L, "rd_abi_entry"):
            raise RadarDepthHipError("%s has no prototype table (rd_abi_entries / rd_abi_entry): it was built before the binding "
                                     "read its prototypes from the library; rebuild it" % LIB_PATH)
        # every prototype comes from the table the compiler derived from include/radar_depth_hip.h (csrc/abi.cpp); this is the
        # only one set by hand
        L.rd_abi_entry.restype = C.c_char_p
        for i in range(L.rd_abi_entries()):
            name, sig = L.rd_abi_entry(i).decode().split(" ")
            ret, args = sig.split(":")
            fn = getattr(L, name)
            fn.restype, fn.argtypes = _CTYPE[ret], [_CTYPE[a] for a in args]
        _lib = L
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
