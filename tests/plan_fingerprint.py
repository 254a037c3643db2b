"""Canonical text of a built execution plan (engine.LateFusionPlan / ResNetPlan / ModulePlan) and the matrix of configurations whose
op lists tests/golden/plan_oplists.json pins (tests/test_plan_oplists_host.py, tests/test_gpu_plan_oplists.py; generator:
tests/golden/make_golden_plan_oplists.py).

One line per op of prep, fwd and bwd: list key, op name, C function, plan.meta family (and descriptor), every argument.  Arguments are
canonicalised so that two processes -- and two revisions of the engine that emit the same launches -- give the same text:
  ints, c_int32 / c_int64, c_float       by value
  a plan stream                          s<index in plan.streams>
  an event                               e<ordinal by first appearance>
  byref(descriptor), a ctypes structure  the bytes of the structure
  a ctypes array                         its canonicalised elements
  a pointer                              p<buffer ordinal by first appearance>+<byte offset>/<buffer bytes>, NULL as `null`
Pointers resolve against the live allocations (plan.keep, the parameter / gradient arenas, the module's parameters and buffers, x_in,
depth_planes, dense_grad_dst), to the widest one that contains the address; an address that resolves to nothing is an error.
Only attributes every revision of the engine has are read (no ctx dicts)."""
import bisect
import contextlib
import ctypes as C
import hashlib
import os
import re
import struct
import types

import torch

_BYREF = type(C.byref(C.c_int()))
_INTS = (C.c_int64, C.c_int32, C.c_uint32, C.c_uint64, C.c_int16, C.c_int8)


class _Canon:
    def __init__(self, plan):
        self.plan = plan
        self.stream_of = {id(s): k for k, s in enumerate(plan.streams)}
        self.event_ids = {id(e) for e in plan.events}
        self.event_ord, self.buf_ord = {}, {}
        spans = {}
        for t in self._tensors(plan):
            st = t.untyped_storage()
            spans[st.data_ptr()] = max(spans.get(st.data_ptr(), 0), st.nbytes())
        self.starts = sorted(spans)
        self.sizes = [spans[s] for s in self.starts]

    @staticmethod
    def _tensors(plan):
        for t in plan.keep:
            if isinstance(t, torch.Tensor):
                yield t
        st = plan.m._ensure_arenas()
        for k in ("arena", "grads", "mom"):
            yield st[k]
        root = plan.m._arena_root()
        for mod in {id(root): root, id(plan.m): plan.m}.values():
            yield from mod.parameters()
            yield from mod.buffers()
        for t in [getattr(plan, "x_in", None), plan.dense_grad_dst] + list(plan.depth_planes or []):      # (a ModulePlan has no x_in)
            if t is not None:
                yield t

    def ptr(self, addr, where):
        if not addr:
            return "null"
        k = bisect.bisect_right(self.starts, addr) - 1
        # widest allocation containing the address: whole storages are disjoint, so it is the one that starts at or below it
        if k < 0 or addr >= self.starts[k] + max(self.sizes[k], 1):
            raise ValueError("%s: pointer %#x resolves to no live allocation of the plan" % (where, addr))
        o = self.buf_ord.setdefault(self.starts[k], len(self.buf_ord))
        return "p%d+%d/%d" % (o, addr - self.starts[k], self.sizes[k])

    def arg(self, a, where):
        if a is None:
            return "null"
        if isinstance(a, (bool, int)):
            return "%d" % int(a)
        if isinstance(a, C.c_float):
            return "f%08x" % struct.unpack("<I", struct.pack("<f", a.value))[0]
        if isinstance(a, _INTS):
            return "%d" % a.value
        if isinstance(a, C.c_void_p):
            if id(a) in self.stream_of:
                return "s%d" % self.stream_of[id(a)]
            if id(a) in self.event_ids:
                return "e%d" % self.event_ord.setdefault(id(a), len(self.event_ord))
            return self.ptr(a.value, where)
        if isinstance(a, _BYREF):
            return "d" + bytes(a._obj).hex()
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                return "[" + ",".join(self.ptr(v, where) for v in a) + "]"
            return "[" + ",".join(self.arg(v, where) for v in a) + "]"
        if isinstance(a, C.Structure):
            return "d" + bytes(a).hex()
        if isinstance(a, torch.Tensor) or hasattr(a, "data_ptr"):
            return ("col:" if not isinstance(a, torch.Tensor) else "") + self.ptr(a.data_ptr(), where)
        if isinstance(a, torch.nn.Module):      # (a folded BatchNorm of evalcoef_jobs)
            return "bn(" + ",".join(self.ptr(t.data_ptr(), where) for t in (a.weight, a.bias, a.running_mean, a.running_var)) + ")"
        if isinstance(a, str):
            return a
        if isinstance(a, (tuple, list)):
            return "(" + ",".join(self.arg(v, where) for v in a) + ")"
        raise TypeError("%s: cannot canonicalise an argument of type %s" % (where, type(a).__name__))


def fingerprint(plan):
    """-> (canonical text, {"prep": n, "fwd": n, "bwd": n})."""
    c = _Canon(plan)
    lines = []
    for key in ("prep", "fwd", "bwd"):
        for k, (name, fn, args) in enumerate(getattr(plan, key)):
            where = "%s[%d] %s" % (key, k, name)
            fam = plan.meta.get(name)
            meta = "-" if fam is None else "%s:%s" % (fam[0], bytes(fam[1]).hex())
            # (the stand-alone split passes carry their tensor's address in their name: split_pieces@<hex>+<channel>)
            cname = re.sub(r"@([0-9a-f]+)", lambda mo: "@" + c.ptr(int(mo.group(1), 16), where), name)
            lines.append(" ".join([key, cname, fn.__name__, meta] + [c.arg(a, where) for a in args]))
    for key in ("pack_jobs", "wino_jobs", "evalcoef_jobs"):
        for k, job in enumerate(getattr(plan, key)):
            lines.append("%s %d %s" % (key, k, c.arg(tuple(job), "%s[%d]" % (key, k))))
    lines.append("reduce_batches %r" % (plan.reduce_batches,))
    lines.append("bwd_segments %r" % (getattr(plan, "bwd_segments", None),))
    lines.append("segment_events %r" % ([len(e) for e in plan.segment_events],))
    lines.append("persistent %r" % ([t.numel() * t.element_size() for t in plan.persistent],))
    lines.append("table_pins %d" % plan.table_pins)
    return "\n".join(lines) + "\n", {key: len(getattr(plan, key)) for key in ("prep", "fwd", "bwd")}


def record(plans):
    """Fixture entry of one configuration (one plan, or the two of a multistage pair)."""
    texts, counts = zip(*[fingerprint(p) for p in plans])
    text = "".join("# plan %d\n%s" % (k, t) for k, t in enumerate(texts))
    return text, {"ops": [c for c in counts], "table_pins": [p.table_pins for p in plans], "sha256": hashlib.sha256(text.encode()).hexdigest()}


# ---------------------------------------------------------------------------------------------------- the matrix
SMALL, LARGE = (2, 97, 161), (16, 450, 800)


def _late(decoder, shape, **kw):
    def build(dev="cpu"):
        from radar_depth_amd.engine import LateFusionPlan
        from radar_depth_amd.model.models import ResNet_latefusion
        torch.manual_seed(0)
        b, h, w = shape
        m = ResNet_latefusion(18, decoder, [h, w], 4, False).to(dev)
        m._ensure_arenas()      # parameters move into the flat arena BEFORE any op captures their addresses
        return [LateFusionPlan(m, b, h, w, dry_run=dev == "cpu", **kw)]
    return build


def _multistage(shape, **kw):
    def build(dev="cpu"):
        from radar_depth_amd import main as hmain
        from radar_depth_amd.engine import LateFusionPlan
        torch.manual_seed(0)
        b, h, w = shape
        args = types.SimpleNamespace(arch="resnet18_multistage_uncertainty_fixs", decoder="upproj", modality="rgbd", pretrained=False)
        model, _ = hmain.create_model(args, [h, w])
        model._ensure_arenas()
        p1 = LateFusionPlan(model.stage1, b, h, w, train=True, dry_run=True, **kw)
        kept = torch.empty(b, 1, h, w)
        p2 = LateFusionPlan(model.stage2, b, h, w, train=True, depth_planes=[kept, p1.pred], x_source=p1.x_in, dense_grad_dst=p1.dpred,
                            dry_run=True, **kw)
        p1.fingerprint_root = model      # (the stages hold their arena owner by weak reference only)
        return [p1, p2]
    return build


def _resnet(layers, modality, decoder, shape, **kw):
    def build(dev="cpu"):
        from radar_depth_amd.engine import ResNetPlan
        from radar_depth_amd.model.models import ResNet
        torch.manual_seed(0)
        b, h, w = shape
        m = ResNet(layers, decoder, [h, w], {"rgb": 3, "rgbd": 4, "d": 1}[modality], False).to(dev)
        m._ensure_arenas()
        return [ResNetPlan(m, b, h, w, dry_run=dev == "cpu", **kw)]
    return build


@contextlib.contextmanager
def _forced_dry_run():
    """ModulePlan has no dry_run argument: build it with LateFusionPlan.__init__ forced to dry_run=True."""
    from radar_depth_amd.engine import LateFusionPlan
    orig = LateFusionPlan.__init__

    def init(self, *a, **kw):
        kw["dry_run"] = True
        orig(self, *a, **kw)
    LateFusionPlan.__init__ = init
    try:
        yield
    finally:
        LateFusionPlan.__init__ = orig


def _module(kind, pick, decoder="upproj", **kw):
    def build(dev="cpu"):
        from radar_depth_amd.engine import ModulePlan
        from radar_depth_amd.model.models import ResNet_latefusion
        torch.manual_seed(0)
        m = ResNet_latefusion(18, decoder, [97, 161], 4, False)
        mod, cin = pick(m)
        with _forced_dry_run():
            return [ModulePlan(m, mod, kind, 2, 24, 40, cin, **kw)]
    return build


def _decoder_cin(m):
    l1 = m.decoder.layer1
    return m.decoder, (l1.upper_branch.conv1.weight.shape[1] if hasattr(l1, "upper_branch") else l1[0].weight.shape[0])


def _configs():
    cfg = {}

    def add(name, build, **env):
        assert name not in cfg
        cfg[name] = (build, env)
    modes = {"fp32": {}, "split": dict(split=True), "bf16": dict(bf16=True), "bf16store": dict(storage="bf16")}
    for mode, kw in modes.items():
        add("late.upproj.small.%s" % mode, _late("upproj", SMALL, train=True, **kw))
    add("late.upproj.large.split", _late("upproj", LARGE, train=True, split=True))
    add("late.upproj.large.fp32", _late("upproj", LARGE, train=True))
    add("late.upproj.small.eval.fp32", _late("upproj", SMALL, train=False))
    add("late.upproj.small.eval.bf16", _late("upproj", SMALL, train=False, bf16=True))
    add("late.upproj.small.split.nojoins", _late("upproj", SMALL, train=True, split=True, segment_joins=False))
    for dec in ("deconv2", "deconv3", "upconv"):
        add("late.%s.small.fp32" % dec, _late(dec, SMALL, train=True))
        add("late.%s.small.split" % dec, _late(dec, SMALL, train=True, split=True))
        add("late.%s.small.eval.fp32" % dec, _late(dec, SMALL, train=False))
    add("late.deconv2.large.split", _late("deconv2", LARGE, train=True, split=True))
    add("multistage.b1.fp32", _multistage((1, 64, 96)))
    add("multistage.b1.split", _multistage((1, 64, 96), split=True))
    add("multistage.b8.large.split", _multistage((8, 450, 800), split=True))
    for mod in ("rgb", "rgbd", "d"):
        for dec in ("upproj", "deconv2"):
            add("resnet18.%s.%s.small.split" % (mod, dec), _resnet(18, mod, dec, SMALL, train=True, split=True))
    add("resnet34.rgbd.upproj.small.split", _resnet(34, "rgbd", "upproj", SMALL, train=True, split=True))
    add("resnet18.rgb.deconv2.small.fp32", _resnet(18, "rgb", "deconv2", SMALL, train=True))
    add("resnet18.rgbd.upproj.small.eval", _resnet(18, "rgbd", "upproj", SMALL, train=False))
    add("resnet18.rgbd.upproj.large.split", _resnet(18, "rgbd", "upproj", LARGE, train=True, split=True))
    picks = {"block.s1": ("block", lambda m: (m.layer1[0], 64), "upproj"),
             "block.s2ds": ("block", lambda m: (m.layer2[0], 64), "upproj"),
             "upproj": ("upproj", lambda m: (m.decoder.layer1, _decoder_cin(m)[1]), "upproj"),
             "decoder.upproj": ("decoder", _decoder_cin, "upproj"),
             "decoder.deconv3": ("decoder", _decoder_cin, "deconv3")}
    for tag, (kind, pick, dec) in picks.items():
        add("module.%s.fp32" % tag, _module(kind, pick, dec))
        add("module.%s.split" % tag, _module(kind, pick, dec, split=True))
    # build-time knobs, one at a time, on the large split upproj plan
    large_split = _late("upproj", LARGE, train=True, split=True)
    add("knob.RD_FUSE_BN_BWD=0", _late("upproj", LARGE, train=True), RD_FUSE_BN_BWD="0")
    add("knob.RD_DEPTH_FORK_ONCE=0", _late("upproj", LARGE, train=True, split=True, segment_joins=False), RD_DEPTH_FORK_ONCE="0")
    for var, vals in (("RD_SPLIT_PRE", ["0"]), ("RD_SPLIT_BNB", ["0", "1", "wino"]), ("RD_WGRAD_PRE", ["1"]), ("RD_WGRAD_SPLIT", ["0"]),
                      ("RD_WGRAD_AFTER_DGRAD", ["0"]), ("RD_WGRAD_REDUCE_BATCH", ["4"]), ("RD_SINGLE_STREAM", ["1"]), ("RD_STREAM_MASK", ["1"]),
                      ("RD_CONV16_SPLIT", ["0"]), ("RD_STEM_SPLIT", ["0"]), ("RD_STEM_WGRAD_BN", ["0"]), ("RD_HEAD_WGRAD_FORK", ["0"]),
                      ("RD_PACK_OVERLAP", ["0"])):
        for v in vals:
            add("knob.%s=%s" % (var, v), large_split, **{var: v})
    return cfg


def _gpu_configs():
    """Real (not dry-run) plans on the MI355X at the tuned table's shape: _tune (table pin + rd_gconv_tune_commit) runs."""
    return {"gpu.late.upproj.large.fp32": (_late("upproj", LARGE, train=True), {}),
            "gpu.late.upproj.large.split": (_late("upproj", LARGE, train=True, split=True), {}),
            "gpu.resnet18.rgbd.deconv2.large.fp32": (_resnet(18, "rgbd", "deconv2", LARGE, train=True), {})}


CONFIGS = _configs()
GPU_CONFIGS = _gpu_configs()
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_oplists.json")
REGENERATE = "python tests/golden/make_golden_plan_oplists.py --dump DIR (at the parent commit and at this one; then diff the two DIR/<configuration>.txt)"
