"""The Adam update against the SGD launch, one job on one MI355X, on the config-2 arena (the late-fusion model's st["total"] floats):
rd_sgd_step, rd_adam_prepare, rd_adam_step (both modes) and, for each streaming launch, a device-to-device copy of the bytes it moves --
five words per element for SGD (p, g, buf read; p, buf written), seven for Adam (p, g, m, v read; p, m, v written).
Every line is the median of REPS timed groups on the device timeline with the fastest and slowest group next to it.  One condition is
checked and reported, not tuned: rd_adam_step reaches at least the fraction of its copy's bandwidth that rd_sgd_step reaches of its own
copy, less the job's run-to-run spread (the largest (slowest - fastest) / median of the timings, as a part of that fraction).
    python tools/bench_adam.py"""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_berhu import H, REPS, W, groups, line, stats  # noqa: E402


def main():
    from radar_depth_amd._lib import check, current_stream, lib, ptr
    from radar_depth_amd.main import create_model
    L = lib()
    arch = types.SimpleNamespace(arch="resnet18_latefusion", decoder="upproj", modality="rgbd", pretrained=False)
    torch.manual_seed(0)
    model = create_model(arch, [H, W]).cuda()
    n = model._ensure_arenas()["total"]
    print("Adam: arena of %d floats (%.1f MB; SGD touches three of them, Adam four = %.1f MB); median of %d groups [fastest .. slowest]"
          % (n, 4 * n / 1e6, 16 * n / 1e6, REPS))
    gen = torch.Generator(device="cuda").manual_seed(1)
    p, g, m = (torch.randn(n, generator=gen, device="cuda") * s for s in (1.0, 1e-2, 1e-2))
    v = torch.rand(n, generator=gen, device="cuda") * 1e-4
    blk = torch.zeros(20, dtype=torch.float64, device="cuda")          # RD_ADAM_BLOCK_WORDS
    blk[:8] = torch.tensor([1e-6, 0.9, 0.999, 1e-8, 1e-2, 0.0, 1.0, 1.0], dtype=torch.float64)   # (a small lr: the arenas stay finite over the timed updates)
    n5, n7 = (5 * n // 2 + 3) // 4 * 4, (7 * n // 2 + 3) // 4 * 4
    src, dst = torch.randn(n7, generator=gen, device="cuda"), torch.empty(n7, device="cuda")
    st = current_stream()

    def sgd():
        check(L.rd_sgd_step(ptr(p), ptr(g), ptr(m), n, 1e-6, 0.9, 1e-4, 1.0, 0, st), "rd_sgd_step")

    def prepare():
        check(L.rd_adam_prepare(ptr(blk), n, 1.0, 0.0, 0, None, 0, None, st), "rd_adam_prepare")

    def adam(mode):
        return lambda: check(L.rd_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), n, mode, ptr(blk), st), "rd_adam_step")

    def copy(k):
        return lambda: dst[:k].copy_(src[:k])

    prepare()
    names = (("sgd", sgd), ("copy5", copy(n5)), ("prepare", prepare), ("adam", adam(0)), ("adamw", adam(1)), ("copy7", copy(n7)))
    t = {name: stats(groups(fn, 50, 10)) for name, fn in names}
    torch.cuda.synchronize()
    print("t = %d after the timed prepare calls; p finite: %s" % (int(blk[5].item()), bool(torch.isfinite(p).all())))
    gbs = lambda words, tt: 4 * words * n / tt[0] / 1e3          # noqa: E731
    line("(a) rd_sgd_step", t["sgd"], "  %.0f GB/s over five arena passes" % gbs(5, t["sgd"]))
    line("(a) copy of 5 n / 2 floats", t["copy5"], "  %.0f GB/s read + written" % gbs(5, t["copy5"]))
    line("(a) rd_adam_prepare", t["prepare"])
    line("(a) rd_adam_step, adam (weight decay in g)", t["adam"], "  %.0f GB/s over seven arena passes" % gbs(7, t["adam"]))
    line("(a) rd_adam_step, adamw (p scaled first)", t["adamw"], "  %.0f GB/s over seven arena passes" % gbs(7, t["adamw"]))
    line("(a) copy of 7 n / 2 floats", t["copy7"], "  %.0f GB/s read + written" % gbs(7, t["copy7"]))
    f_sgd, f_adam = t["copy5"][0] / t["sgd"][0], t["copy7"][0] / max(t["adam"][0], t["adamw"][0])
    spread = max((t[k][2] - t[k][1]) / t[k][0] for k in ("sgd", "copy5", "adam", "adamw", "copy7"))
    print("    rd_sgd_step runs at %.3f of its copy's bandwidth, rd_adam_step (the slower mode) at %.3f of its own; spread %.3f of the "
          "timings (%s the kernel condition: %.3f >= %.3f)" % (f_sgd, f_adam, spread, "meets" if f_adam >= f_sgd * (1 - spread) else "MISSES",
                                                             f_adam, f_sgd * (1 - spread)))
    alone = t["prepare"][0] + t["adamw"][0]
    extra = alone - t["sgd"][0]
    print("    stand-alone time of the Adam launches = %.1f us, %.1f us more than rd_sgd_step" % (alone, extra))


if __name__ == "__main__":
    main()
