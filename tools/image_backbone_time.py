#!/usr/bin/env python3
"""Time ``image_backbone.ResNet.forward`` (the 2D image backbone in front of the detector: mmdet.ResNet depth 50, base 16, every BatchNorm
frozen) on an MI355X and write the report profiles/image_backbone.txt keeps.

Input: the shipped configuration on 6 x 50 x 480 x 480 (the test pipeline) and 6 x 20 x 480 x 480 (the training pipeline) images, float32
and uint8 (uint8 with the data preprocessor's mean / std in the stem); the seeded weights of tests/image_backbone_util.py.

Two sides, whole calls through Python, HIP events:

* ``ResNet.forward``;
* the torch fp32 composition of the same stages on the same device: ``F.conv2d`` with the BatchNorm folded into weight and bias,
  ``F.relu``, ``F.max_pool2d``, contiguous and ``channels_last`` (the faster one is reported), under ``no_grad``.  Where torch's
  convolution does not run on the machine the report says so and gives our side only.

Per side: the median of --blocks blocks of --reps calls after a warm-up block, the sides alternating, the inputs rotating over two image
tensors (each larger than the last-level cache), with the range of the blocks.  Then launch kind by launch kind on each stage's own
shapes at the 50-view batch: the entry point through ctypes and its torch counterpart, every call on the next of 2 or 8 sets of buffers
(a set is out of the last-level cache when its turn comes again), the bytes the launch must move (input, output, residual, once
each), the share of the 8 TB/s HBM rate that is, and for the 3x3 launches the share of the 157 TF fp32 matrix peak.
Last, the 4x rule's ratios of tests/test_gpu_image_backbone.py (device error / float32 chain's error against the float64 chain, per
level).  ``--trace`` runs a few forwards and nothing else: the workload of a ``rocprofv3 --kernel-trace --stats`` run of its own.

Usage (on a GPU):  python tools/image_backbone_time.py [--blocks 5] [--reps 3] [--out profiles/image_backbone.txt]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import alternate      # noqa: E402

H = W = 480
PEAK_TF, PEAK_TBS = 157.0, 8.0


def spread(values, digits=0):
    return f"(min {min(values):.{digits}f}, max {max(values):.{digits}f})"


def folded(net, dev):
    """{name: (weight, bias)} of every convolution with its BatchNorm folded in, on ``dev``."""
    from proxytransformation_amd.sparse import bn_fold
    out = {}

    def put(name, conv, bn):
        scale, shift = bn_fold(bn)
        out[name] = ((conv.weight.detach() * scale.view(-1, 1, 1, 1)).to(dev).contiguous(), shift.to(dev).contiguous())
    put("stem", net.conv1, net.bn1)
    for s in range(net.num_stages):
        for b, blk in enumerate(getattr(net, f"layer{s + 1}")):
            p = f"layer{s + 1}.{b}."
            put(p + "1", blk.conv1, blk.bn1)
            put(p + "2", blk.conv2, blk.bn2)
            put(p + "3", blk.conv3, blk.bn3)
            if blk.downsample is not None:
                put(p + "d", blk.downsample[0], blk.downsample[1])
    return out


def torch_forward(net, fw, x, channels_last):
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x = F.max_pool2d(F.relu(F.conv2d(x, *fw["stem"], stride=2, padding=3)), 3, 2, 1)
    outs = []
    for s in range(net.num_stages):
        for b, blk in enumerate(getattr(net, f"layer{s + 1}")):
            p = f"layer{s + 1}.{b}."
            idn = F.conv2d(x, *fw[p + "d"], stride=blk.stride) if p + "d" in fw else x
            y = F.relu(F.conv2d(x, *fw[p + "1"]))
            y = F.relu(F.conv2d(y, *fw[p + "2"], stride=blk.stride, padding=1))
            x = F.relu(F.conv2d(y, *fw[p + "3"]) + idn)
        outs.append(x)
    return [o.contiguous() for o in outs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_backbone.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_backbone_time.py measures on a GPU: none found")
    from proxytransformation_amd import _abi
    from tests import image_backbone_util as U
    dev = torch.device("cuda:0")
    net = U.build_backbone().to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    if args.trace:
        x = torch.randn((6 * 50, 3, H, W), generator=g, device=dev)
        for _ in range(3):
            net(x)
        torch.cuda.synchronize()
        return
    fw = folded(net, dev)
    lines = [f"ResNet(depth=50, base_channels=16), every BatchNorm folded; {torch.cuda.get_device_name(0)}; images of {H} x {W}",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides "
             "alternating, two image tensors in rotation",
             "torch: F.conv2d (BatchNorm folded) + F.relu + F.max_pool2d, fp32, no_grad; contiguous and channels_last, the faster is compared"]
    for views in (50, 20):
        N = 6 * views
        xs = [torch.randn((N, 3, H, W), generator=g, device=dev) for _ in range(2)]
        x8 = [(x * 40 + 128).clamp(0, 255).to(torch.uint8) for x in xs]
        turn = {"n": 0}

        def rot(pool):
            turn["n"] += 1
            return pool[turn["n"] & 1]

        sides = {"hip": lambda: net(rot(xs)), "hip uint8": lambda: net(rot(x8), mean=U.MEAN, std=U.STD)}
        torch_ok = None
        try:
            with torch.no_grad():
                a, b = net(xs[0]), torch_forward(net, fw, xs[0], False)
                errs = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(a, b)]
                torch_forward(net, fw, xs[0], True)
                del a, b
            torch.cuda.synchronize()
            torch_ok = errs

            def side(cl):
                def run():
                    with torch.no_grad():
                        return torch_forward(net, fw, rot(xs), cl)
                return run
            sides["torch"], sides["torch channels_last"] = side(False), side(True)
        except Exception as e:      # noqa: BLE001  (torch's convolution library may be unable to run here: recorded, not hidden)
            lines.append(f"  torch's convolution did not run on this machine ({type(e).__name__}: {str(e)[:120]}): our side only")
        med, t, _ = alternate(sides, args.blocks, args.reps)
        lines.append(f"6 x {views} x {H} x {W} ({N} images, {N * 3 * H * W * 4 / 1e6:.0f} MB of float32 pixels):")
        for k in sides:
            lines.append(f"  {k:22s} {med[k] / 1e3:9.2f} ms {spread([v / 1e3 for v in t[k]], 2)}")
        if torch_ok is not None:
            best = min(med["torch"], med["torch channels_last"])
            lines.append(f"  torch (faster layout) / hip = {best / med['hip']:.2f}" + ("   BEHIND torch" if med["hip"] > best else "")
                         + f";  max |hip - torch| / max |torch| per level: {', '.join(f'{e:.1e}' for e in torch_ok)}")
        del xs, x8

    # launch kind by launch kind at the 50-view batch
    lib, st = _abi.lib(), torch.cuda.current_stream(dev).cuda_stream
    N = 300
    prep = net._prepare(dev)
    new = lambda *shape: torch.randn(shape, generator=g, device=dev)      # noqa: E731
    p = lambda t_: t_.data_ptr()      # noqa: E731
    lines.append(f"launch by launch at {N} images (hip: the entry point through ctypes; torch: F.conv2d with the folded BatchNorm + the "
                 "epilogue's torch ops, the faster layout); every call takes the next of 2 (layer1, layer2) or 8 (layer3, layer4) sets of buffers, "
                 "so that a set is out of the 256 MB last-level cache when its turn comes again; MB = input + output + residual once each "
                 f"(the weight is negligible); % HBM = MB / time against {PEAK_TBS:.0f} TB/s; 3x3: share of the {PEAK_TF:.0f} TF fp32 matrix "
                 "peak:")
    total = 0.0
    sel = {"i": 0}
    R = lambda sets: sets[sel["i"] % len(sets)]      # noqa: E731  (this call's set of a rotated buffer)

    def report(name, times, hfn, tfn, mbytes, gflop=0.0):
        nonlocal total
        def turn(fn):
            def run():
                sel["i"] += 1
                return fn()
            return run
        sides = {"hip": turn(hfn)}
        if tfn is not None:
            try:
                with torch.no_grad():
                    tfn(False), tfn(True)
                torch.cuda.synchronize()
                sides["torch"] = turn(lambda: tfn(False))
                sides["torch cl"] = turn(lambda: tfn(True))
            except Exception:      # noqa: BLE001
                pass
        m2, t2, _ = alternate(sides, args.blocks, args.reps)
        total += m2["hip"] * times
        line = (f"  {name:34s} x{times:<2d} hip {m2['hip']:9.1f} us {spread(t2['hip']):22s} {mbytes:7.0f} MB "
                f"{100 * mbytes / m2['hip'] / PEAK_TBS:5.1f} % HBM")
        if gflop:
            line += f"  {gflop:6.1f} GFLOP {100 * gflop / m2['hip'] * 1e3 / PEAK_TF:5.1f} % of peak"
        if "torch" in m2:
            best = min(m2["torch"], m2["torch cl"])
            line += f"   torch {best:9.1f} us  torch / hip {best / m2['hip']:5.2f}" + ("  BEHIND torch" if m2["hip"] > best else "")
        lines.append(line)

    with torch.no_grad():
        C0 = net.stem_channels
        h = w = 120
        x = [new(N, 3, H, W) for _ in range(2)]
        out = [torch.empty((N, C0, h, w), device=dev) for _ in range(2)]
        cl = lambda sets: [t_.contiguous(memory_format=torch.channels_last) for t_ in sets]      # noqa: E731
        xcl = cl(x)
        report("stem 7x7 + BN + ReLU + max-pool", 1,
               lambda: lib.ptx_conv_stem(p(R(x)), 0, N, H, W, p(prep["stem"]), C0, p(prep["bn1"][0]), p(prep["bn1"][1]), 1, None, None, p(R(out)), st),
               lambda on: F.max_pool2d(F.relu(F.conv2d(R(xcl) if on else R(x), *fw["stem"], stride=2, padding=3)), 3, 2, 1),
               (x[0].numel() + out[0].numel()) * 4 / 1e6)
        del x, xcl, out
        inpl = C0
        for s in range(net.num_stages):
            blocks = prep["stages"][s]
            d0, d1 = blocks[0], blocks[1]
            sd = d0["stride"]
            ho, wo = (h - 1) // sd + 1, (w - 1) // sd + 1
            pl, oc = d0["planes"], d0["out"]
            pre = f"layer{s + 1}."
            nset = 2 if s < 2 else 8
            sets = lambda *shape: [new(*shape) for _ in range(nset)]      # noqa: E731
            xin, t1, t2, idn, o = sets(N, inpl, h, w), sets(N, pl, h, w), sets(N, pl, ho, wo), sets(N, oc, ho, wo), sets(N, oc, ho, wo)
            xo, t1o = sets(N, oc, ho, wo), sets(N, pl, ho, wo)
            mb = lambda *ts: sum(t_[0].numel() for t_ in ts) * 4 / 1e6      # noqa: E731
            xin_cl, t1_cl, t2_cl, idn_cl, xo_cl, t1o_cl = (cl(t_) for t_ in (xin, t1, t2, idn, xo, t1o))
            nb = len(blocks)
            report(f"{pre}0 1x1 {inpl}->{pl} @{h}", 1,
                   lambda: lib.ptx_conv1x1(p(R(xin)), N, inpl, h, w, p(d0["w1"]), pl, 1, p(d0["bn1"][0]), p(d0["bn1"][1]), None, 1, p(R(t1)), st),
                   lambda on: F.relu(F.conv2d(R(xin_cl) if on else R(xin), *fw[pre + "0.1"])), mb(xin, t1))
            report(f"{pre}0 3x3 {pl} s{sd} @{h}", 1,
                   lambda: lib.ptx_conv3x3(p(R(t1)), N, pl, h, w, p(d0["w2"]), sd, p(d0["bn2"][0]), p(d0["bn2"][1]), None, 1, p(R(t2)), st),
                   lambda on: F.relu(F.conv2d(R(t1_cl) if on else R(t1), *fw[pre + "0.2"], stride=sd, padding=1)), mb(t1, t2),
                   2.0 * N * ho * wo * pl * pl * 9 / 1e9)
            report(f"{pre}0 downsample 1x1 {inpl}->{oc} s{sd}", 1,
                   lambda: lib.ptx_conv1x1(p(R(xin)), N, inpl, h, w, p(d0["wd"]), oc, sd, p(d0["bnd"][0]), p(d0["bnd"][1]), None, 0, p(R(idn)), st),
                   lambda on: F.conv2d(R(xin_cl) if on else R(xin), *fw[pre + "0.d"], stride=sd), mb(xin, idn))
            report(f"{pre}* 1x1 {pl}->{oc} + residual @{ho}", nb,
                   lambda: lib.ptx_conv1x1(p(R(t2)), N, pl, ho, wo, p(d0["w3"]), oc, 1, p(d0["bn3"][0]), p(d0["bn3"][1]), p(R(idn)), 1, p(R(o)), st),
                   lambda on: F.relu(F.conv2d(R(t2_cl) if on else R(t2), *fw[pre + "0.3"]) + (R(idn_cl) if on else R(idn))), mb(t2, idn, o))
            report(f"{pre}1+ 1x1 {oc}->{pl} @{ho}", nb - 1,
                   lambda: lib.ptx_conv1x1(p(R(xo)), N, oc, ho, wo, p(d1["w1"]), pl, 1, p(d1["bn1"][0]), p(d1["bn1"][1]), None, 1, p(R(t1o)), st),
                   lambda on: F.relu(F.conv2d(R(xo_cl) if on else R(xo), *fw[pre + "1.1"])), mb(xo, t1o))
            report(f"{pre}1+ 3x3 {pl} s1 @{ho}", nb - 1,
                   lambda: lib.ptx_conv3x3(p(R(t1o)), N, pl, ho, wo, p(d1["w2"]), 1, p(d1["bn2"][0]), p(d1["bn2"][1]), None, 1, p(R(t2)), st),
                   lambda on: F.relu(F.conv2d(R(t1o_cl) if on else R(t1o), *fw[pre + "1.2"], padding=1)), mb(t1o, t2),
                   2.0 * N * ho * wo * pl * pl * 9 / 1e9)
            del xin, t1, t2, idn, o, xo, t1o, xin_cl, t1_cl, t2_cl, idn_cl, xo_cl, t1o_cl
            inpl, h, w = oc, ho, wo
    lines.append(f"  sum of the launches of a forward (x counts applied): hip {total / 1e3:.2f} ms")

    # the 4x rule of tests/test_gpu_image_backbone.py
    lines.append("4x rule (tests/test_gpu_image_backbone.py): max|device - f64| / max|f64| over max|float32 chain - f64| / max|f64|, per level:")
    for case in sorted(U.MODULE_CASES):
        ref = U.reference(case)
        m = ref["net"].to(dev)
        got = [o.cpu().numpy() for o in m(ref["imgs"].to(dev))]
        m.cpu()
        ratios = [U.err(d, f64) / U.err(f32, f64) for d, f32, f64 in zip(got, ref["f32"], ref["f64"])]
        e32 = [U.err(f32, f64) for f32, f64 in zip(ref["f32"], ref["f64"])]
        lines.append(f"  {case:20s} ratios {', '.join(f'{r:.2f}' for r in ratios)}   (float32 chain: {', '.join(f'{e:.1e}' for e in e32)})")
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
