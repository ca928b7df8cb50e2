#!/usr/bin/env python3
"""Time a training pass of ``image_backbone.ResNet(differentiable=True)`` (forward + backward of the kernels of stages 2 to 4, every
BatchNorm frozen) on an MI355X and write the report profiles/image_backbone_train.txt keeps.

Input: the shipped configuration on 6 x 50 x 480 x 480 float32 images (``--views 20``: the training pipeline's 6 x 20, for a machine on
which the torch side does not fit); the seeded weights of tests/image_backbone_util.py.

Two sides, whole calls through Python, HIP events (tools/sparse_conv_time.alternate: the median of --blocks blocks of --reps calls after a
warm-up block, the sides alternating, two image tensors in rotation):

* ours: a simulated optimizer step (an in-place update of every trainable kernel, which bumps its version), then ``ResNet.forward`` in
  grad mode -- the prepared operands are rebuilt inside it -- and ``torch.autograd.backward`` of the levels with fixed level gradients.
  The data gradient's transposed weight is re-laid inside every backward call (csrc/conv2d_bwd.hip: k_conv_wt), so it is in the time too;
* torch: the same update, then the fp32 composition under autograd -- ``F.conv2d`` with the BatchNorm folded into weight and bias (the
  fold is recomputed from the updated kernels inside the timed call, as ours is), the stem and layer1 under ``no_grad``, contiguous and
  ``channels_last``, the faster one is compared -- and the same backward.

Then launch by launch at the same batch: dx alone and dweight alone of each distinct (kind, widths, stride, map) of stages 2 to 4 through
ctypes (no epilogue: ``g`` is read as it is) against ``aten.convolution_backward`` with the matching output mask on the same operands,
contiguous and ``channels_last``, every call on the next of 2 or 8 sets of buffers.  Last, the 4x rule's ratios of
tests/test_gpu_image_backbone_grad.py on its module cases.

Usage (on a GPU):  python tools/image_backbone_train_time.py [--views 50] [--blocks 3] [--reps 2] [--out profiles/image_backbone_train.txt]
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
from image_backbone_time import spread      # noqa: E402
from sparse_conv_time import alternate      # noqa: E402

H = W = 480


def torch_step(net, x, grads, channels_last):
    """The torch composition of one training pass: fold, frozen part under no_grad, trainable tail under autograd, backward."""
    from proxytransformation_amd.sparse import bn_fold

    def conv(x, c, bn, stride=1, padding=0):
        scale, shift = bn_fold(bn)
        return F.conv2d(x, c.weight * scale.view(-1, 1, 1, 1), shift, stride=stride, padding=padding)

    def block(x, blk):
        idn = conv(x, blk.downsample[0], blk.downsample[1], blk.stride) if blk.downsample is not None else x
        y = F.relu(conv(x, blk.conv1, blk.bn1))
        y = F.relu(conv(y, blk.conv2, blk.bn2, blk.stride, 1))
        return F.relu(conv(y, blk.conv3, blk.bn3) + idn)

    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    outs = []
    with torch.no_grad():
        x = F.max_pool2d(F.relu(conv(x, net.conv1, net.bn1, 2, 3)), 3, 2, 1)
        for blk in net.layer1:
            x = block(x, blk)
        outs.append(x)
    for s in range(1, net.num_stages):
        for blk in getattr(net, f"layer{s + 1}"):
            x = block(x, blk)
        outs.append(x)
    torch.autograd.backward(outs[1:], [g.contiguous(memory_format=torch.channels_last) if channels_last else g for g in grads[1:]])
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_backbone_train.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_backbone_train_time.py measures on a GPU: none found")
    from proxytransformation_amd import _abi
    from tests import image_backbone_util as U
    dev = torch.device("cuda:0")
    net = U.build_backbone(differentiable=True).to(dev)
    names = net._trainable_names()
    weights = [net.get_parameter(n) for n in names]
    g = torch.Generator(device=dev).manual_seed(0)
    N = 6 * args.views
    lines = [f"ResNet(depth=50, base_channels=16, frozen_stages=1, differentiable=True); {torch.cuda.get_device_name(0)}; {N} images of {H} x {W} "
             f"(6 x {args.views} views), float32",
             f"whole calls through Python, HIP events, median of {args.blocks} blocks of {args.reps} calls after a warm-up block, sides "
             "alternating, two image tensors in rotation",
             f"a call = a simulated optimizer step (in-place update of the {len(names)} trainable kernels), forward in grad mode (operands rebuilt), "
             "backward of the levels with fixed level gradients"]
    xs = [torch.randn((N, 3, H, W), generator=g, device=dev) for _ in range(2)]
    grads = [torch.randn((N,) + s, generator=g, device=dev) * 1e-3 for s in net.level_shapes(H, W)]
    turn = {"n": 0}

    def rot(pool):
        turn["n"] += 1
        return pool[turn["n"] & 1]

    def update():
        with torch.no_grad():
            for w in weights:
                w.mul_(1.0)                                 # bumps the version: the prepared operands are stale
                w.grad = None

    def ours():
        update()
        levels = net(rot(xs))
        torch.autograd.backward(levels[1:], grads[1:])

    def ours_forward_only():
        with torch.no_grad():
            net(rot(xs))

    sides = {"hip forward + backward": ours, "hip eval forward": ours_forward_only}
    try:
        for cl in (False, True):
            update()
            torch_step(net, xs[0], grads, cl)
        torch.cuda.synchronize()
        t_grads = [w.grad.clone() for w in weights]
        update()
        torch.autograd.backward(net(xs[0])[1:], grads[1:])  # the same images as the torch side's
        torch.cuda.synchronize()
        dev_err = max(float((w.grad - t).abs().max() / t.abs().max()) for w, t in zip(weights, t_grads))
        lines.append(f"max over the kernels of max |hip grad - torch grad| / max |torch grad| = {dev_err:.1e}")

        def side(cl):
            def run():
                update()
                torch_step(net, rot(xs), grads, cl)
            return run
        sides["torch forward + backward"], sides["torch channels_last f + b"] = side(False), side(True)
    except Exception as e:      # noqa: BLE001  (recorded, not hidden)
        lines.append(f"  the torch side did not run at this shape ({type(e).__name__}: {str(e)[:160]}): our side only")
    med, t, _ = alternate(sides, args.blocks, args.reps)
    for k in sides:
        lines.append(f"  {k:28s} {med[k] / 1e3:9.2f} ms {spread([v / 1e3 for v in t[k]], 2)}")
    if "torch forward + backward" in med:
        best = min(med["torch forward + backward"], med["torch channels_last f + b"])
        hip = med["hip forward + backward"]
        lines.append(f"  torch (faster layout) / hip = {best / hip:.2f}" + ("   BEHIND torch" if hip > best else ""))
    update()
    del xs, grads
    torch.cuda.empty_cache()

    if not args.skip_launches:
        lib, st = _abi.lib(), torch.cuda.current_stream(dev).cuda_stream
        lines.append(f"launch by launch at {N} images, no epilogue (hip: ptx_conv1x1_bwd / ptx_conv3x3_bwd through ctypes with only dx, or only "
                     "dweight, asked for -- dx includes the weight's re-layout; torch: aten.convolution_backward with the matching output mask, "
                     "the faster of contiguous and channels_last); every call takes the next of 2 (layer2) or 8 (layer3, layer4) sets of buffers:")
        sel = {"i": 0}
        R = lambda sets: sets[sel["i"] % len(sets)]      # noqa: E731
        new = lambda *shape: torch.randn(shape, generator=g, device=dev)      # noqa: E731
        p = lambda t_: t_.data_ptr()      # noqa: E731
        cl = lambda sets: [t_.contiguous(memory_format=torch.channels_last) for t_ in sets]      # noqa: E731
        behind = []
        totals = {"hip": 0.0, "torch": 0.0}

        def report(name, times, KS, cin, cout, h, w, sd, nset):
            ho, wo = (h - 1) // sd + 1, (w - 1) // sd + 1
            x, gout = [new(N, cin, h, w) for _ in range(nset)], [new(N, cout, ho, wo) for _ in range(nset)]
            wt = new(cout, cin, KS, KS) * 0.05
            wop = wt.reshape(cout, cin).contiguous() if KS == 1 else wt.permute(0, 2, 3, 1).contiguous()
            dx, dw = [torch.empty_like(t_) for t_ in x], torch.empty_like(wop)
            nbytes = int(lib.ptx_conv_bwd_workspace_bytes(KS, N, cin, cout, h, w, sd))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            S = lib.ptx_conv_dweight_chunks(KS, N, cin, cout, h, w, sd)
            x_cl, g_cl, w_cl = cl(x), cl(gout), wt.contiguous(memory_format=torch.channels_last)

            def hip(want_dx):
                def run():
                    sel["i"] += 1
                    a = (p(R(gout)), None, None, 0, p(R(x)), N, cin, h, w, p(wop)) + ((cout, sd) if KS == 1 else (sd,))
                    a += (None, None, p(R(dx)) if want_dx else None, 0, None if want_dx else p(dw), p(ws), nbytes, st)
                    rc = (lib.ptx_conv1x1_bwd if KS == 1 else lib.ptx_conv3x3_bwd)(*a)
                    assert rc == 0, lib.ptx_last_error()
                return run

            def tor(want_dx, on):
                def run():
                    sel["i"] += 1
                    return torch.ops.aten.convolution_backward(R(g_cl) if on else R(gout), R(x_cl) if on else R(x), w_cl if on else wt, None,
                                                               [sd, sd], [KS // 2, KS // 2], [1, 1], False, [0, 0], 1,
                                                               [want_dx, not want_dx, False])
                return run

            for want_dx in (True, False):
                sides = {"hip": hip(want_dx)}
                try:
                    tor(want_dx, False)(), tor(want_dx, True)()
                    torch.cuda.synchronize()
                    sides["torch"], sides["torch cl"] = tor(want_dx, False), tor(want_dx, True)
                except Exception:      # noqa: BLE001
                    pass
                m2, t2, _ = alternate(sides, args.blocks, args.reps)
                kind = "dx     " if want_dx else f"dweight"
                line = f"  {name:34s} x{times:<2d} {kind} hip {m2['hip']:9.1f} us {spread(t2['hip']):22s}"
                if not want_dx:
                    line += f" S={S:<5d}"
                totals["hip"] += m2["hip"] * times
                if "torch" in m2:
                    best = min(m2["torch"], m2["torch cl"])
                    totals["torch"] += best * times
                    line += f"   torch {best:9.1f} us  torch / hip {best / m2['hip']:5.2f}"
                    if m2["hip"] > best:
                        line += "  BEHIND torch"
                        behind.append(f"{name} {kind.strip()}")
                lines.append(line)

        inpl, h, w = 64, 120, 120
        for s in range(1, net.num_stages):
            pl, oc = net.base_channels * 2 ** s, net.base_channels * 2 ** s * 4
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            nb = net.stage_blocks[s]
            nset = 2 if s < 2 else 8
            pre = f"layer{s + 1}."
            report(f"{pre}0 1x1 {inpl}->{pl} @{h}", 1, 1, inpl, pl, h, w, 1, nset)
            report(f"{pre}0 3x3 {pl} s2 @{h}", 1, 3, pl, pl, h, w, 2, nset)
            report(f"{pre}0 downsample 1x1 {inpl}->{oc} s2", 1, 1, inpl, oc, h, w, 2, nset)
            report(f"{pre}* 1x1 {pl}->{oc} @{ho}", nb, 1, pl, oc, ho, wo, 1, nset)
            report(f"{pre}1+ 1x1 {oc}->{pl} @{ho}", nb - 1, 1, oc, pl, ho, wo, 1, nset)
            report(f"{pre}1+ 3x3 {pl} s1 @{ho}", nb - 1, 3, pl, pl, ho, wo, 1, nset)
            inpl, h, w = oc, ho, wo
        lines.append(f"  sum over a backward (x counts applied; layer2.0's two dx are not computed in a real pass): hip {totals['hip'] / 1e3:.2f} ms, "
                     f"torch {totals['torch'] / 1e3:.2f} ms")
        lines.append("  launch classes behind torch: " + ("; ".join(behind) if behind else "none"))

    # the 4x rule of tests/test_gpu_image_backbone_grad.py
    lines.append("4x rule (tests/test_gpu_image_backbone_grad.py): per module case, over the trainable kernels, the worst of max|device grad - f64| / "
                 "max|f64| over max|float32 host - f64| / max|f64| (both hosts replay the device's ReLU masks):")
    for case, (kw, shape) in (("shipped-5x64x80", (dict(differentiable=True), (5, 3, 64, 80))),
                              ("deep-2x64x64", (dict(U.DEEP, frozen_stages=1, differentiable=True), (2, 3, 64, 64)))):
        m = U.build_backbone(**kw).to(dev)
        imgs = U.make_images(shape).to(dev)
        levels = m(imgs)
        gen = torch.Generator().manual_seed(5)
        gl = [torch.randn(tuple(l.shape), generator=gen).to(dev) for l in levels]
        torch.autograd.backward([l for l in levels if l.requires_grad], [g_ for l, g_ in zip(levels, gl) if l.requires_grad])
        masks = m.relu_masks(imgs)
        f64, f32 = m.grad_host(imgs, gl, np.float64, masks), m.grad_host(imgs, gl, np.float32, masks)
        ratios = {n: U.err(m.get_parameter(n).grad.cpu().numpy(), f64[n]) / U.err(f32[n], f64[n]) for n in f64}
        worst = max(ratios, key=ratios.get)
        e32 = [U.err(f32[n], f64[n]) for n in f64]
        lines.append(f"  {case:18s} {len(ratios)} kernels: worst ratio {ratios[worst]:.2f} ({worst}), median {float(np.median(list(ratios.values()))):.2f}; "
                     f"float32 host's own error {min(e32):.1e} .. {max(e32):.1e}")
    text_out = "\n".join(lines) + "\n"
    print(text_out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out)


if __name__ == "__main__":
    main()
