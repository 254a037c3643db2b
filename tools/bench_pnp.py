"""PnP-Depth refinement (main.HipPnPInference) against what it stands next to, one job on one MI355X, b = 1 at 450x800,
resnet18_latefusion / upproj:
  (1) a HipInference frame and HipPnPInference at iters = 1 (the same op list) and iters = 5, all as hipGraph replays, timed in
      alternating groups of the same job;
  (2) the primitives alone, as plain launches: rear(), grad(), update();
  (3) rd_act_gate_t and rd_pnp_update alone on the largest decoder shape ([1,240,400,16]: the output of decoder.layer4) and on an
      UpProj half of it (a 16-channel slice of 32), against a device copy of the same bytes; rd_pnp_update on the latent itself;
  (4) the same five-iteration loop written with torch autograd over the oracle's modules on the GPU, wall clock with one final
      synchronisation per loop.
Every device line is the median of REPS timed groups on the device timeline with the fastest and slowest group next to it.
Conditions, checked and reported, not tuned:
  (a) iters = 1 is within the job's run-to-run spread of HipInference;
  (b) (T5 - T1) / 4 is at most rear() + grad() + update() measured alone, plus the spread: the loop adds no synchronisation or idle gap;
  (c) iters = 5 is faster than the torch loop.
    python tools/bench_pnp.py [--no-torch] [--out profiles/r17_pnp.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

B, H, W = 1, 450, 800
ITERS, ALPHA = 5, 0.01
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


def stats(out):
    return float(np.median(out)), min(out), max(out)


def line(name, t, extra=""):
    say("%-66s %10.1f us  [%.1f .. %.1f]%s" % (name, t[0], t[1], t[2], extra))


def alternating(fns, inner, warmup):
    """REPS groups of each callable, interleaved (the same job, the same minutes) -> one list of group times per callable."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(REPS):
        for k, fn in enumerate(fns):
            out[k].append(group(fn, inner))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17_pnp.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_pnp.py measures on an MI355X"
    from radar_depth_amd._lib import current_stream, lib
    from radar_depth_amd.main import HipInference, HipPnPInference
    from radar_depth_amd.model.models import ResNet_latefusion
    from radar_depth_amd.synthetic import make_batch, procedural_fill_
    L = lib()
    dev = "cuda:0"
    say("PnP-Depth refinement, %s, b = %d at %dx%d, resnet18_latefusion / upproj, alpha = %g" % (torch.cuda.get_device_name(0), B, H, W, ALPHA))
    net = ResNet_latefusion(18, "upproj", [H, W], 4, False)
    procedural_fill_(net)
    net = net.to(dev).eval()
    x, _ = make_batch(B, H, W, 7)
    x = x.to(dev)
    inf = HipInference(net, B, H, W)
    one = HipPnPInference(net, B, H, W, iters=1, alpha=ALPHA)
    five = HipPnPInference(net, B, H, W, iters=ITERS, alpha=ALPHA)
    say("valid pixels of the sparse plane: %d" % int((x[:, 3] > 0).sum().item()))

    say("")
    say("(1) whole frames, hipGraph replay, alternating groups of 10")
    t_inf, t_one, t_five = [stats(v) for v in alternating([lambda: inf(x), lambda: one(x), lambda: five(x)], 10, 3)]
    line("HipInference", t_inf)
    line("HipPnPInference iters = 1", t_one)
    line("HipPnPInference iters = %d" % ITERS, t_five)
    assert five.graph is not None and one.graph is not None and inf.graph is not None
    say("    losses of the last frame: %s" % " ".join("%.5f" % v for v in five.losses.tolist()))
    plain = inf(x).clone()
    say("    iters = 1 bit-identical to HipInference: %s; max |refined - plain| = %.4g" %
        (bool(torch.equal(one(x), plain)), float((five(x) - plain).abs().max().item())))

    say("")
    say("(2) the primitives alone, plain launches, groups of 10")
    prim = HipPnPInference(net, B, H, W, iters=ITERS, alpha=ALPHA, use_graph=False)
    prim.front(x)
    t_front, t_rear, t_grad, t_upd = [stats(v) for v in alternating([lambda: prim.front(x), prim.rear, prim.grad, prim.update], 10, 3)]
    line("front(x)", t_front)
    line("rear()", t_rear)
    line("grad()  (loss, loss gradient, %d ops of pnp_bwd)" % len(prim.plan.pnp_bwd), t_grad)
    line("update()", t_upd)

    say("")
    say("(3) the two kernels alone, groups of 50")
    st = current_stream()
    alpha = torch.full((1,), ALPHA, device=dev)
    for name, M, Cc, ld in (("[1,240,400,16] whole tensors", 240 * 400, 16, 16), ("[1,240,400,16] as a half of 32 channels", 240 * 400, 16, 32),
                            ("the latent [1,15,25,256]", 15 * 25, 256, 256)):
        dy, y, out = [torch.randn(M, ld, device=dev) for _ in range(3)]
        p = lambda t: C.c_void_p(t.data_ptr())
        nbytes = 3 * M * Cc * 4
        src, dst = torch.empty(nbytes // 8, dtype=torch.float32, device=dev), torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
        t_gate, t_updk, t_copy = [stats(v) for v in alternating(
            [lambda: L.rd_act_gate_t(0, p(dy), ld, p(y), ld, p(out), ld, M, Cc, 1, st), lambda: L.rd_pnp_update(p(out), ld, p(dy), ld, M, Cc, p(alpha), st),
             lambda: dst.copy_(src)], 50, 3)]
        say("  %s: %.2f MB read + written per call" % (name, nbytes / 1e6))
        line("    rd_act_gate_t", t_gate, "  %.0f GB/s" % (nbytes / t_gate[0] / 1e3))
        line("    rd_pnp_update", t_updk, "  %.0f GB/s" % (nbytes / t_updk[0] / 1e3))
        line("    device copy of the same bytes", t_copy, "  %.0f GB/s" % (nbytes / t_copy[0] / 1e3))

    t_torch = None
    if not args.no_torch:
        say("")
        say("(4) the same loop in torch autograd over the oracle's modules on the GPU, wall clock, one synchronisation per loop")
        import pnp_ref
        from oracle.criteria import MaskedL1Loss
        from oracle.models import ResNet_latefusion as OracleNet
        ref = OracleNet(18, "upproj", [H, W], 4, False)
        procedural_fill_(ref)
        ref = ref.to(dev).eval()
        sparse = x[:, 3:4].contiguous()

        def torch_loop():
            out, _ = pnp_ref.loop(ref, MaskedL1Loss(), x, sparse, ITERS, ALPHA)
            torch.cuda.synchronize()
            return out
        for _ in range(3):
            want = torch_loop()
        walls = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            torch_loop()
            walls.append((time.perf_counter() - t0) * 1e6)
        t_torch = stats(walls)
        line("torch loop, iters = %d" % ITERS, t_torch)
        got = five(x)
        say("    refined prediction against the torch loop's: rel err %.3g (max norm)" % float(((got - want).abs().max() / want.abs().max()).item()))

    say("")
    say("conditions")
    spread = lambda t: t[2] - t[1]
    sp = max(spread(t_inf), spread(t_one))
    say("  (a) iters = 1 within the spread of HipInference: |%.1f - %.1f| = %.1f us against a spread of %.1f us: %s"
        % (t_one[0], t_inf[0], abs(t_one[0] - t_inf[0]), sp, "met" if abs(t_one[0] - t_inf[0]) <= sp else "MISSED"))
    per, alone = (t_five[0] - t_one[0]) / (ITERS - 1), t_rear[0] + t_grad[0] + t_upd[0]
    sp = max(spread(t_five), spread(t_one)) / (ITERS - 1) + spread(t_rear) + spread(t_grad) + spread(t_upd)
    say("  (b) (T%d - T1) / %d = %.1f us against rear + grad + update alone = %.1f us (+ spread %.1f us): %s"
        % (ITERS, ITERS - 1, per, alone, sp, "met" if per <= alone + sp else "MISSED"))
    if t_torch is not None:
        say("  (c) iters = %d: %.1f us against the torch loop's %.1f us, %.2fx: %s"
            % (ITERS, t_five[0], t_torch[0], t_torch[0] / t_five[0], "met" if t_five[0] < t_torch[0] else "MISSED"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
