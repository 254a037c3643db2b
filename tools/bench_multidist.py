"""Distance-interval metrics (rd_depth_metrics_multidist + rd_meter_update_multidist) against what they stand next to, one job on one
MI355X, b = 16 at 450x800:
  (a) rd_depth_metrics and rd_depth_metrics_multidist on the same pair (whole-tensor form), on the dataset's sparse targets and on a
      dense target with every interval in every wave (the binning kernel's worst case);
  (b) the per-frame form (frames = 16) and one frame (frames = 1, what validate() at batch 1 issues), each with its meter update;
  (c) ten rd_depth_metrics passes on the same tensors -- the price of a direct port of the reference's loop over the intervals;
  (d) the reference's algorithm itself in torch on the GPU (a boolean-mask gather, an emptiness test and ten blocking float()
      conversions per interval), in wall-clock time;
  (e) a device copy of the bytes the binning reads, for the fraction of the copy bandwidth;
  (f) a HipInference frame (b = 1), for the validation-side condition;
  (g) the fused config-2 training step (resnet18_latefusion b = 16, split operands) with metrics=True and with metrics="multidist",
      timed in alternating groups of the same job.
Every device line is the median of REPS timed groups on the device timeline with the fastest and slowest group next to it.  The
conditions are checked and reported, not tuned.
    python tools/bench_multidist.py [--no-step] [--out profiles/r16_multidist.txt]"""
import argparse
import ctypes as C
import math
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, H, W = 16, 450, 800
REPS = 15
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def group(fn, inner):
    """us per call of one group of ``inner`` calls, on the device timeline"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3


def groups(fn, inner, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [group(fn, inner) for _ in range(REPS)]


def stats(out):
    return float(np.median(out)), min(out), max(out)


def line(name, t, extra=""):
    say("%-66s %10.1f us  [%.1f .. %.1f]%s" % (name, t[0], t[1], t[2], extra))


def torch_loop(output, target, edges):
    """The reference's evaluate as it would run on the GPU: one pass per interval, every number fetched with a blocking float()."""
    valid = target > 0
    out = []
    for k, hi in enumerate(edges):
        lo = 0. if k == 0 else edges[k - 1]
        hi = math.inf if k == len(edges) - 1 else hi
        m = (target >= lo) & (target <= hi) & valid
        empty = bool(torch.sum(m) == 0)
        o, t = output[m], target[m]
        d = (o - t).abs()
        mse = float((d ** 2).mean())
        row = [mse, math.sqrt(mse), float(d.mean()), float((torch.log(o) / math.log(10) - torch.log(t) / math.log(10)).abs().mean()), float((d / t).mean())]
        r = torch.max(o / t, t / o)
        row += [float((r < 1.25 ** p).float().mean()) for p in (1, 2, 3)]
        inv = (1 / o - 1 / t).abs()
        row += [math.sqrt((inv ** 2).mean()), float(inv.mean())]
        out.append((row, empty))
    return out


def resource_lines():
    path = os.path.join(REPO, "radar_depth_amd", "csrc", "build", "metrics_multidist.hip.resource.txt")
    if not os.path.exists(path):
        return ["    (no compiler resource report next to the objects)"]
    out, name = [], None
    for ln in open(path):
        text = ln.split("remark:")[-1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
        if text.startswith("Function Name:"):
            name, vals = text.split(":", 1)[1].strip(), {}
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill", "LDS Size [bytes/block]"):
            if text.startswith(key + ":"):
                vals[key] = text.split(":", 1)[1].strip()
        if text.startswith("LDS Size") and name and "md_partial" in name:
            out.append("    %s: VGPRs %s, LDS %s B/block, scratch %s B/lane, VGPR spills %s, %s waves/SIMD" %
                       (name, vals.get("VGPRs"), vals.get("LDS Size [bytes/block]"), vals.get("ScratchSize [bytes/lane]"), vals.get("VGPRs Spill"),
                        vals.get("Occupancy [waves/SIMD]")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r16_multidist.txt"))
    args = ap.parse_args()
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    from radar_depth_amd.evaluation.metrics import DIST_INTERVAL
    from radar_depth_amd.synthetic import make_batch
    L = lib()
    say("distance-interval metrics: b=%d %dx%d, ten intervals; median of %d groups [fastest .. slowest]" % (B, H, W, REPS))
    say("  binning kernel, compiler's resource report:")
    for ln in resource_lines():
        say(ln)
    xs, t = make_batch(B, H, W, 1234)
    xs, t = xs.cuda(), t.cuda()
    pred = (t + torch.randn_like(t).abs() * 3 + 0.5).contiguous()
    dense_t = (torch.rand_like(t) * 109.5 + 0.5).contiguous()
    dense_o = (dense_t * (torch.rand_like(t) * 1.7 + 0.5)).contiguous()
    n, hw = pred.numel(), H * W
    f64 = lambda *k: torch.zeros(*k, dtype=torch.float64, device="cuda")      # noqa: E731
    st = current_stream()
    tiles = L.rd_loss_tiles(C.c_int64(n))
    ws10, s10 = f64(10 * tiles), f64(10)
    nws = max(int(L.rd_depth_metrics_multidist_workspace_floats(f, n // f, 10)) for f in (1, B))
    wsm, sm = f64(nws // 2), f64(B, 10, 10)
    meter, last, valid = f64(10, 12), f64(10, 10), torch.zeros(10, dtype=torch.int32, device="cuda")
    wgt = torch.full((1,), float(B), dtype=torch.float64, device="cuda")

    def plain(o=pred, tg=t):
        check(L.rd_depth_metrics(ptr(o), ptr(tg), C.c_int64(n), ptr(ws10), ptr(s10), st), "rd_depth_metrics")

    def binning(o=pred, tg=t, frames=1):
        check(L.rd_depth_metrics_multidist(ptr(o), ptr(tg), frames, n // frames, None, 10, ptr(wsm), ptr(sm), st), "rd_depth_metrics_multidist")

    def update(rows=1):
        check(L.rd_meter_update_multidist(ptr(sm), rows, 10, ptr(wgt) if rows == 1 else None, None, 1, ptr(meter), ptr(last), ptr(valid), st),
              "rd_meter_update_multidist")

    def one_frame():
        check(L.rd_depth_metrics_multidist(ptr(pred), ptr(t), 1, hw, None, 10, ptr(wsm), ptr(sm), st), "rd_depth_metrics_multidist")
        update(1)

    def ten(o=pred, tg=t):
        for _ in range(10):
            plain(o, tg)

    copy_dst = torch.empty(2 * n, device="cuda")
    copy_src = torch.cat([pred.flatten(), t.flatten()])
    k = {}
    for name, fn, inner in (("plain", plain, 50), ("bin", binning, 50), ("plain_dense", lambda: plain(dense_o, dense_t), 50),
                            ("bin_dense", lambda: binning(dense_o, dense_t), 50), ("bin_frames", lambda: binning(frames=B), 50),
                            ("bin_frames_dense", lambda: binning(dense_o, dense_t, B), 50), ("update1", lambda: update(1), 50),
                            ("update16", lambda: update(B), 50), ("one_frame", one_frame, 50), ("ten", ten, 10),
                            ("ten_dense", lambda: ten(dense_o, dense_t), 10), ("copy", lambda: copy_dst.copy_(copy_src), 50)):
        k[name] = stats(groups(fn, inner, 10))
    binning()
    torch.cuda.synchronize()
    say("  sparse pair: %d of %d pixels valid, per interval %s" % (int((t > 0).sum()), n, [int(v) for v in sm[0, :, 0].cpu().numpy()]))
    gbs = lambda us: "  %.0f GB/s" % (8 * n / us / 1e3)      # noqa: E731
    line("(e) device copy of the bytes read (2 x %d floats)" % n, k["copy"], gbs(k["copy"][0]) + " read")
    line("(a) rd_depth_metrics, sparse targets", k["plain"], gbs(k["plain"][0]))
    line("(a) rd_depth_metrics_multidist, sparse targets", k["bin"], gbs(k["bin"][0]) + ", %.2f of the copy's rate" % (k["copy"][0] / k["bin"][0]))
    line("(a) rd_depth_metrics, dense targets", k["plain_dense"], gbs(k["plain_dense"][0]))
    line("(a) rd_depth_metrics_multidist, dense targets (worst case)", k["bin_dense"], gbs(k["bin_dense"][0]) + ", %.2f of the copy's rate" %
         (k["copy"][0] / k["bin_dense"][0]))
    line("(b) per-frame form, frames = %d, sparse" % B, k["bin_frames"])
    line("(b) per-frame form, frames = %d, dense" % B, k["bin_frames_dense"])
    line("(b) rd_meter_update_multidist, 1 row", k["update1"])
    line("(b) rd_meter_update_multidist, %d rows" % B, k["update16"])
    line("(b) one frame (hw = %d): binning + update" % hw, k["one_frame"])
    line("(c) ten rd_depth_metrics passes, sparse", k["ten"])
    line("(c) ten rd_depth_metrics passes, dense", k["ten_dense"])
    for tag, a, b in (("sparse", "bin", "ten"), ("dense", "bin_dense", "ten_dense")):
        say("    %s: one binning call / ten passes = %.2f (%s the condition: less than the ten passes)" %
            (tag, k[a][0] / k[b][0], "meets" if k[a][0] < k[b][0] else "MISSES"))
    # (d) the reference's loop in torch, wall clock (it synchronises about 120 times per call)
    wall = {}
    for tag, o, tg in (("sparse", pred, t), ("dense", dense_o, dense_t)):
        torch_loop(o, tg, DIST_INTERVAL)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            torch_loop(o, tg, DIST_INTERVAL)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        wall[tag] = stats(ts)
        line("(d) the reference's loop in torch (wall clock), %s" % tag, wall[tag])
    if not args.no_step:
        from radar_depth_amd.main import HipInference, HipTrainStep, create_model
        mk = lambda: create_model(types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False), [H, W]).cuda()      # noqa: E731
        torch.manual_seed(0)
        inf = HipInference(mk().eval(), 1, H, W, use_graph=False)
        x1 = xs[:1].contiguous()
        k["inf"] = stats(groups(lambda: inf(x1), 10, 5))
        line("(f) HipInference frame, b = 1, plain launches", k["inf"])
        frac = k["one_frame"][0] / k["inf"][0]
        say("    binning + update of one frame / HipInference frame = %.4f (%s the 0.1 condition)" % (frac, "meets" if frac < 0.1 else "MISSES"))
        del inf
        steps, order = {}, (True, "multidist")
        for m in order:
            torch.manual_seed(0)
            steps[m] = HipTrainStep(mk(), B, H, W, lr=0.01, momentum=0.9, weight_decay=1e-4, operands="split", metrics=m)
            for _ in range(5):
                steps[m].step(xs, t)
        torch.cuda.synchronize()
        out = {m: [] for m in order}
        for _ in range(REPS):                                   # alternating groups: both steps see the same drift of the machine
            for m in order:
                out[m].append(group(lambda: steps[m].step(xs, t), 5))
        s1, s2 = stats(out[True]), stats(out["multidist"])
        line("(g) fused step, metrics=True", s1, "  %.0f samples/s" % (B / s1[0] * 1e6))
        line("(g) fused step, metrics='multidist'", s2, "  %.0f samples/s" % (B / s2[0] * 1e6))
        # the step's own prediction decides how many intervals a wave meets: time the two added launches on it
        p = steps["multidist"].plan.pred
        k["bin_step"] = stats(groups(lambda: (binning(p, t), update(1)), 50, 10))
        line("(g) the two added launches on the step's own prediction", k["bin_step"])
        added = k["bin_step"][0]
        frac = added / s1[0]
        say("    binning + update / fused step = %.4f (%s the 0.1 condition)" % (frac, "meets" if frac < 0.1 else "MISSES"))
        spread = max(s1[2] - s1[1], s2[2] - s2[1])
        over = s2[0] - (s1[0] + added)
        say("    multidist step - (metrics=True step + %.1f us) = %+.1f us; run-to-run spread of the job %.1f us (%s the condition)"
            % (added, over, spread, "meets" if over <= spread else "MISSES"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
