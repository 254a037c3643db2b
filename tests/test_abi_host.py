"""No-GPU checks of the drop-in boundary: the C-ABI library loads and exports every symbol declared in
include/radar_depth_hip.h; argument validation returns error codes (no compute); the plugin surface
(parse_command / create_model / constructors) mirrors the reference's names, defaults and error behaviour."""
import ctypes as C
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from radar_depth_amd.build import build
    build(verbose=False)
    from radar_depth_amd._lib import lib
    return lib()


def test_every_declared_symbol_is_exported(L):
    hdr = open(os.path.join(REPO, "include", "radar_depth_hip.h")).read()
    names = sorted(set(re.findall(r"\b(rd_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 45
    assert [n for n in names if not hasattr(L, n)] == []
    assert L.rd_abi_version() == 1
    # the compiled prototype table (csrc/abi.cpp) names exactly the declared entry points, and lib() bound every one of them from it
    table = dict(L.rd_abi_entry(i).decode().split(" ") for i in range(L.rd_abi_entries()))
    assert sorted(table) == names and len(table) == L.rd_abi_entries()
    assert L.rd_abi_entry(-1) is None and L.rd_abi_entry(L.rd_abi_entries()) is None
    for n, sig in table.items():
        assert len(getattr(L, n).argtypes) == len(sig.split(":")[1]), n
    assert {n: table[n] for n in ("rd_fill", "rd_sgd_step", "rd_uniform_sparsify", "rd_wino_packed_bytes", "rd_last_error", "rd_loss_tiles",
                                  "rd_optable_set_word")} == {
        "rd_fill": "i:plfp", "rd_sgd_step": "i:ppplffffip", "rd_uniform_sparsify": "i:pliiildpLLpplpp", "rd_wino_packed_bytes": "l:iii",
        "rd_last_error": "s:", "rd_loss_tiles": "i:l", "rd_optable_set_word": "i:piiL"}


def test_arguments_travel_as_the_prototype_says(L):
    """A bare number is converted through the compiled prototype (a 64-bit count is not cut to 32 bits), and a ctypes scalar of
    another type than the prototype's is refused before the call."""
    n = (1 << 33) + 5
    assert L.rd_loss_tiles(n) == L.rd_loss_tiles(C.c_int64(n)) == 1024 and L.rd_loss_tiles(5) == 1
    with pytest.raises(C.ArgumentError):
        L.rd_fill(None, C.c_int32(1), 0.0, None)
    with pytest.raises(C.ArgumentError):
        L.rd_fill(None, 1, C.c_double(0.0), None)


def test_no_prototype_is_set_outside_the_binding():
    """Source lint: the prototypes come from the library's own table in radar_depth_amd/_lib.py; no other Python file assigns
    .restype or .argtypes (each such line was a second copy of a prototype)."""
    import glob
    files = [os.path.join(REPO, "bench.py")]
    for d in ("radar_depth_amd", "tools", "tests"):
        files += glob.glob(os.path.join(REPO, d, "**", "*.py"), recursive=True)
    assert len(files) > 30
    offenders = []
    for f in sorted(files):
        if os.path.relpath(f, REPO) == os.path.join("radar_depth_amd", "_lib.py"):
            continue
        for n, line in enumerate(open(f), 1):
            if re.search(r"\.(restype|argtypes)\s*=[^=]", line.split("#")[0]):
                offenders.append("%s:%d" % (os.path.relpath(f, REPO), n))
    assert offenders == []


def test_argument_validation_without_gpu(L):
    from radar_depth_amd import convdesc as cd
    d = cd.conv_fwd(2, 9, 7, 24, 8, 3, 1, 1)            # Cin not a multiple of 16
    assert L.rd_gconv_stat_tiles(C.byref(d)) < 0
    assert b"Cin" in L.rd_last_error()
    assert L.rd_gconv(C.byref(cd.conv_fwd(2, 9, 7, 32, 8, 3, 1, 1)), None, None, None, None, 0, None, None) == -1
    assert L.rd_sgd_step(None, None, None, C.c_int64(4), C.c_float(0.1), C.c_float(0.9), C.c_float(0.0), C.c_float(1.0), 0, None) == -1
    d = cd.upproj_fwd(2, 15, 25, 256, 256)
    assert L.rd_gconv_stat_tiles(C.byref(d)) > 0 and L.rd_wgrad_workspace_floats(C.byref(d)) > 0


def test_plugin_surface():
    from radar_depth_amd import main as hmain, utils
    from radar_depth_amd.model import models, multistage_model
    a = utils.parse_command(["-a", "resnet18_latefusion", "-d", "upproj", "-m", "rgbd", "--data", "nuscenes", "--no-pretrain", "-b", "16"])
    assert (a.arch, a.decoder, a.modality, a.batch_size, a.pretrained, a.lr, a.momentum, a.weight_decay) == \
        ("resnet18_latefusion", "upproj", "rgbd", 16, False, 0.01, 0.9, 1e-4)
    assert models.Decoder.names == ["deconv2", "deconv3", "upconv", "upproj"]
    m = hmain.create_model(a, [450, 800])
    assert isinstance(m, models.ResNet_latefusion) and len(m.state_dict()) == 325
    a.arch = "resnet18_multistage_uncertainty_fixs"
    m2, lw = hmain.create_model(a, [450, 800])
    assert isinstance(m2, multistage_model.ResNet_multistage) and lw["w_smooth"] == 0.1
    assert [n for n, _ in m2.named_parameters()][:2] == ["w_stage1", "w_stage2"] and len(m2.state_dict()) == 652
    with pytest.raises(ValueError, match="Unknown model"):
        hmain.create_model(types.SimpleNamespace(arch="nope", decoder="upproj", modality="rgbd", pretrained=False), [450, 800])
    with pytest.raises(RuntimeError):
        models.ResNet_latefusion(19, "upproj", [450, 800])
    with pytest.raises(AssertionError):
        models.ResNet_latefusion(18, "upproj", [450, 800], in_channels=3, pretrained=False)
    with pytest.raises(AssertionError):
        models.choose_decoder("deconv9x", 256)
    with pytest.raises(ValueError, match="pretrained latefusion"):
        multistage_model.ResNet_multistage(18, "upproj", [450, 800], True)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(torch.zeros(1, 4, 450, 800))
    opt = torch.optim.SGD(m.parameters(), 0.01)
    assert utils.adjust_learning_rate(opt, 7, 0.01) == pytest.approx(0.001) and opt.param_groups[0]["lr"] == pytest.approx(0.001)


def test_checkpoint_wire_format(tmp_path):
    """the reference's .pth.tar payload round-trips between the HIP-backed modules and the
    reference-shaped (oracle) modules: identical keys, shapes and values, multistage shape filtering included."""
    from oracle.models import ResNet_latefusion as ORef
    from oracle.multistage_model import ResNet_multistage as OMulti
    from radar_depth_amd import utils
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.model.multistage_model import ResNet_multistage
    from radar_depth_amd.synthetic import procedural_fill_
    src = ORef(18, "upproj", [97, 161], 4, False)
    procedural_fill_(src)
    opt = torch.optim.SGD(src.parameters(), 0.01, momentum=0.9, weight_decay=1e-4)
    path = utils.save_checkpoint({"args": None, "epoch": 3, "arch": "resnet18_latefusion", "model_state_dict": src.state_dict(),
                                  "best_result": None, "optimizer_state_dict": opt.state_dict()}, True, 3, str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "model_best.pth.tar"))
    ck = torch.load(path, map_location="cpu", weights_only=False)
    m = ResNet_latefusion(18, "upproj", [97, 161], 4, False)
    missing, unexpected = m.load_state_dict(ck["model_state_dict"], strict=False)     # main.py:208,251 use strict=False
    assert not missing and not unexpected
    for (k, a), (k2, b) in zip(m.state_dict().items(), src.state_dict().items()):
        assert k == k2 and torch.equal(a, b)
    # multistage: stage 1 loads the late-fusion checkpoint directly, stage 2 drops the shape-mismatched depth stem
    ms = ResNet_multistage(18, "upproj", [97, 161], False)
    ms.stage1.load_state_dict(ck["model_state_dict"])
    filt = ms.filter_state_dict(dict(ck["model_state_dict"]), ms.stage2.state_dict())
    assert "conv1_depth.weight" not in filt and len(filt) == 324
    ms.stage2.load_state_dict(filt, strict=False)
    assert torch.equal(ms.stage2.conv3.weight, src.conv3.weight)
    # and back: a HIP-module checkpoint loads into the reference-shaped module
    om = OMulti(18, "upproj", [97, 161], False)
    om.load_state_dict(ms.state_dict())


def test_authors_checkpoint_payload_loads(tmp_path):
    """The authors' .pth.tar files pickle an argparse.Namespace under `args` and an `evaluation.metrics.Result` under
    `best_result` (main.py:358-374).  torch >= 2.6 refuses both under its weights_only default and the Result class lives at
    the REFERENCE's module path: utils.load_checkpoint must read such a file, and ResNet_multistage(pretrained=True) must
    initialise both stages from it (multistage_model.py:34-61)."""
    import argparse
    import sys
    import types

    from oracle.models import ResNet_latefusion as ORef
    from radar_depth_amd import utils
    from radar_depth_amd.evaluation.metrics import Result
    from radar_depth_amd.model.multistage_model import ResNet_multistage
    from radar_depth_amd.synthetic import procedural_fill_
    # write the file the way the reference does: Result pickled as evaluation.metrics.Result
    pkg, mod = types.ModuleType("evaluation"), types.ModuleType("evaluation.metrics")

    class RefResult(object):
        def __init__(self):
            self.rmse, self.mae, self.delta1 = 5.25, 2.5, 0.875
    RefResult.__module__, RefResult.__qualname__, RefResult.__name__ = "evaluation.metrics", "Result", "Result"
    mod.Result, pkg.metrics = RefResult, mod
    src = ORef(18, "upproj", [97, 161], 4, False)
    procedural_fill_(src)
    root = tmp_path / "proj"
    (root / "pretrained").mkdir(parents=True)
    path = str(root / "pretrained" / "resnet18_latefusion.pth.tar")
    sys.modules["evaluation"], sys.modules["evaluation.metrics"] = pkg, mod
    try:
        torch.save({"args": argparse.Namespace(arch="resnet18_latefusion", lr=0.01), "epoch": 19, "arch": "resnet18_latefusion",
                    "model_state_dict": src.state_dict(), "best_result": RefResult(), "optimizer_state_dict": None}, path)
    finally:
        del sys.modules["evaluation"], sys.modules["evaluation.metrics"]
    with pytest.raises(Exception):
        torch.load(path, map_location="cpu")              # what the round-1 code did: rejected by the weights_only default
    ck = utils.load_checkpoint(path)
    assert isinstance(ck["best_result"], Result) and ck["best_result"].rmse == 5.25 and ck["args"].arch == "resnet18_latefusion"
    assert "evaluation.metrics" not in sys.modules        # the alias does not leak
    ms = ResNet_multistage(18, "upproj", [97, 161], pretrained=True, project_root=str(root))
    assert torch.equal(ms.stage1.conv1_depth.weight, src.conv1_depth.weight)
    assert torch.equal(ms.stage2.layer4[1].conv2.weight, src.layer4[1].conv2.weight)
    assert ms.stage2.conv1_depth.weight.shape == (16, 2, 7, 7)        # shape-filtered: keeps its own init


def test_result_container_semantics():
    """Result keeps the reference's attribute names / update() argument order (evaluation/metrics.py:10-31)."""
    import numpy as np
    from radar_depth_amd.evaluation.metrics import AverageMeter, Result
    r = Result()
    assert (r.irmse, r.imae, r.mse, r.rmse, r.mae, r.absrel, r.lg10, r.delta1, r.delta2, r.delta3, r.data_time, r.gpu_time) == (0,) * 12
    r.set_to_worst()
    assert r.rmse == np.inf and r.irmse == np.inf and r.lg10 == np.inf and r.delta1 == 0 and r.gpu_time == 0
    r.update(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)
    assert (r.irmse, r.imae, r.mse, r.rmse, r.mae, r.absrel, r.lg10, r.delta1, r.delta2, r.delta3) == tuple(range(1, 11))
    assert r.gpu_time == 11 and r.data_time == 12
    am = AverageMeter()
    am.update(r, 0.5, 0.25, n=2)
    am.update(r, 1.5, 0.75, n=2)
    avg = am.average()
    assert avg.rmse == 4 and avg.delta3 == 10 and avg.gpu_time == 1.0 and avg.data_time == 0.5


def test_every_kernel_barrier_goes_through_rd_sync():
    """Source lint for the LDS race fixed in round 2 (csrc/common.h): hipcc's wait-count pass dropped the lgkmcnt(0) in front of a
    loop-header s_barrier, so a bare __syncthreads() is not a safe LDS barrier in this library.  Every barrier in the kernels must be
    rd_sync() (explicit s_waitcnt lgkmcnt(0) + __syncthreads()); the only __syncthreads() left is the one inside rd_sync itself."""
    import glob
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "radar_depth_amd", "csrc")
    offenders = []
    for f in sorted(glob.glob(os.path.join(root, "*.hip")) + glob.glob(os.path.join(root, "*.h")) + glob.glob(os.path.join(root, "*.cpp"))):
        for n, line in enumerate(open(f), 1):
            code = line.split("//")[0]
            if re.search(r"\b__syncthreads\s*\(", code):
                offenders.append("%s:%d" % (os.path.basename(f), n))
    assert len(offenders) == 1 and offenders[0].startswith("common.h:"), offenders
    common = open(os.path.join(root, "common.h")).read()
    assert re.search(r"void rd_sync\(\)\s*\{\s*asm volatile\(\"s_waitcnt lgkmcnt\(0\)\"[^;]*;\s*__syncthreads\(\);", common)
    assert 'asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"' in common          # glds_wait


def test_no_kernel_spills_vector_registers():
    """ISA audit: no kernel of the library spills VGPRs to scratch (round 2: the input-parity-group instantiations of
    gconv_kernel spilled 40-65 VGPRs -- 264 B of scratch per lane inside the stride-2 convolutions).  Reads hipcc's
    -Rpass-analysis=kernel-resource-usage report that radar_depth_amd/build.py keeps next to every object."""
    import importlib.util
    from radar_depth_amd.build import OBJ, build
    build(verbose=False)
    spec = importlib.util.spec_from_file_location("audit_resources", os.path.join(REPO, "tools", "audit_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n, bad = 0, []
    for f in sorted(os.listdir(OBJ)):
        if not f.endswith(".resource.txt"):
            continue
        for name, r in mod.parse(os.path.join(OBJ, f)):
            n += 1
            if r.get("VGPRs Spill", 0) > 0 or r.get("ScratchSize [bytes/lane]", 0) > 0:
                bad.append((f, name, r.get("VGPRs Spill", 0), r.get("ScratchSize [bytes/lane]", 0)))
    assert n > 150, "resource reports missing (%d kernels seen): rebuild with python -m radar_depth_amd.build --force" % n
    assert not bad, bad


# ---- the shared host layer of the convolution files (csrc/conv_host.h): cache key, plan-all switches, error texts, source lint
def _info(fn, d, n):
    out = (C.c_int32 * n)()
    assert fn(C.byref(d), out) == 0, fn.__name__
    return list(out)


def test_stale_tile_begin_does_not_make_a_second_plan(L):
    """The tile_begin fields are filled by the library: a caller's stale values in them must reach the plan already cached for the
    descriptor -- same state, same answers -- not plan it a second time."""
    from radar_depth_amd import convdesc as cd
    d = cd.conv_fwd(3, 23, 37, 64, 128, 3, 1, 1)            # (a shape no other test plans)
    assert L.rd_gconv_plan_state(C.byref(d), 1) == 0
    queries = ((L.rd_gconv_plan_info, 10), (L.rd_gconv_bf16_plan_info, 8), (L.rd_gconv_split_plan_info, 8))
    want = [_info(fn, d, n) for fn, n in queries]
    tiles = L.rd_gconv_stat_tiles(C.byref(d))
    assert tiles > 0 and L.rd_gconv_plan_state(C.byref(d), 1) == 2
    e = cd.RdConvDesc()
    C.memmove(C.byref(e), C.byref(d), C.sizeof(d))
    for i in range(4):
        e.phase[i].tile_begin = 1000 + 17 * i
    assert bytes(e) != bytes(d)
    assert L.rd_gconv_plan_state(C.byref(e), 1) == 2
    assert [_info(fn, e, n) for fn, n in queries] == want and L.rd_gconv_stat_tiles(C.byref(e)) == tiles


def test_plan_all_switches_return_the_previous_value_and_drop_stale_plans(L):
    """rd_gconv_split_plan_all / rd_gconv_bf16p_plan_all: each call returns the setting it replaces, and a descriptor served only
    under "all" is answered 0 / 1 / 0 across the toggles -- the answer cached under one setting does not outlive it."""
    from radar_depth_amd import convdesc as cd
    d = cd.conv_fwd(2, 19, 27, 32, 32, 3, 1, 1)             # 3x3 with 32 channels a side: left to rd_gconv unless "all"
    first = L.rd_gconv_split_plan_all(0)
    try:
        assert L.rd_gconv_split_supported(C.byref(d)) == 0
        assert L.rd_gconv_split_plan_all(1) == 0 and L.rd_gconv_split_supported(C.byref(d)) == 1
        assert L.rd_gconv_split_plan_all(1) == 1 and L.rd_gconv_split_supported(C.byref(d)) == 1
        assert L.rd_gconv_split_plan_all(0) == 1 and L.rd_gconv_split_supported(C.byref(d)) == 0
    finally:
        L.rd_gconv_split_plan_all(first)

    def persistent(desc):           # (+ 2000 in the chunk slot marks the persistent kernel)
        out = (C.c_int32 * 8)()
        assert L.rd_gconv_bf16_plan_info_t(1, C.byref(desc), out) == 0
        return (1 if out[2] >= 2000 else 0), out[0]
    p = cd.conv_fwd(2, 15, 25, 64, 64, 3, 1, 1)             # small-spatial 3x3: 128-pixel tiles, which the planner rule leaves out
    first = L.rd_gconv_bf16p_plan_all(0)
    try:
        assert persistent(p)[0] == 0
        assert L.rd_gconv_bf16p_plan_all(1) == 0 and persistent(p) == (1, 1)
        assert L.rd_gconv_bf16p_plan_all(0) == 1 and persistent(p)[0] == 0
    finally:
        L.rd_gconv_bf16p_plan_all(first)


def test_descriptor_error_texts(L):
    """rd_last_error() of the descriptor checks, byte for byte, through the three entry points that validate with messages."""
    from radar_depth_amd import convdesc as cd

    def bad(edit, Cin=32):
        d = cd.conv_fwd(2, 11, 17, Cin, 32, 3, 1, 1)
        edit(d)
        return d

    def set_n_phases(d): d.n_phases = 0
    def set_tap(d): d.phase[0].dh[4] = 5
    def set_empty(d): d.phase[0].lw = 0
    cases = [(bad(set_n_phases), "n_phases=0"), (bad(set_tap), "tap 4 of phase 0 outside its declared range"),
             (bad(lambda d: None, Cin=24), "Cin=24 must be a multiple of 16, ldi=24 of 4"), (bad(set_empty), "empty phase 0")]
    out = (C.c_int32 * 10)()
    for d, text in cases:
        assert L.rd_gconv_plan_info(C.byref(d), out) == -1 and L.rd_last_error() == b"gconv: " + text.encode()
        assert L.rd_gconv_bf16_plan_info(C.byref(d), out) == -1 and L.rd_last_error() == b"gconv_bf16: " + text.encode()
        assert L.rd_gconv_tune_pin(C.byref(d), 1, None) == -1 and L.rd_last_error() == b"gconv: " + text.encode()


def test_conv_host_code_lives_in_one_place():
    """Source lint over csrc/*.hip: the dynamic-LDS attribute is set by launch_dyn_lds alone (occ_cfg of gconv.hip, a diagnostic,
    sets it without the per-device bit on purpose), plan caches are PlanCache (no string-keyed map of a file's own), and no file
    declares a function that another .hip defines -- those declarations live in conv_internal.h."""
    import glob
    root = os.path.join(REPO, "radar_depth_amd", "csrc")
    files = sorted(glob.glob(os.path.join(root, "*.hip")))
    assert len(files) > 25
    proto = re.compile(r"^(?:namespace\s+\w+\s*\{\s*)?(?!static\b|extern\b|template\b|typedef\b|using\b|return\b|namespace\b)[A-Za-z_][\w:<>\*& ]*?\b(\w+)\([^;{}]*\)\s*;", re.M)
    offenders = []
    for f in files:
        name, text = os.path.basename(f), open(f).read()
        code = re.sub(r"//[^\n]*", "", text)
        attr = [m.start() for m in re.finditer("hipFuncAttributeMaxDynamicSharedMemorySize", code)]
        if name == "gconv.hip":
            assert len(attr) == 1 and "occ_cfg" in code[code.rfind("template", 0, attr[0]):attr[0]]
        elif attr:
            offenders.append((name, "sets the dynamic-LDS attribute itself"))
        # (the slot table of gconv_split.hip is a string-keyed map of device pointers, not a plan cache)
        if len(re.findall(r"unordered_map<std::string", code)) > (1 if name == "gconv_split.hip" else 0):
            offenders.append((name, "string-keyed map"))
        for m in proto.finditer(code):
            if not re.search(r"^[A-Za-z_][\w:<>\*& ]*\b%s\([^;{}]*\)\s*\{" % re.escape(m.group(1)), code, re.M):
                offenders.append((name, "declares %s, defined elsewhere" % m.group(1)))
    assert offenders == []
    internal = open(os.path.join(root, "conv_internal.h")).read()
    for fn in ("launch_slab_reduce", "launch_bn_bwd_coeffs", "wgrad_bf16_reduce_shape", "launch_conv16", "gemm1_split_supported"):
        assert len(re.findall(r"\b%s\(" % fn, internal)) == 1
