#!/usr/bin/env python3
"""Time forward + backward of the sparse convolution (proxytransformation_amd/sparse.py with ``differentiable=True``:
ptx_sparse_conv3d + ptx_sparse_conv3d_bwd) and write the report profiles/sparse_conv_bwd.txt keeps.

Same input and the same three layers as tools/sparse_conv_time.py: six room clouds of 100 000 points through ``quantize`` at 1 cm;
  stem      3 -> 64, k3 stride 2, on the 1 cm rows
  64x64     64 -> 64, k3 stride 1, on the rows of tensor stride 8
  512x512   512 -> 512, k3 stride 1, on the rows of tensor stride 64
Both ``feats`` and ``weight`` require grad; one call = forward + ``torch.autograd.grad`` of a fixed upstream gradient.  Baseline: the torch
composition a user could write from ``nbr`` -- per offset ``index_select`` + ``mm`` + ``index_add_``, autograd doing the backward (the
per-offset index lists are made once, outside the timing).  Same GPU, HIP events around blocks of --reps calls, the two sides
alternating from block to block, block 0 a warm-up, reported = median of the blocks.  The dweight launches (k_sparse_dweight +
k_sparse_slab_sum) are timed apart through the library call with only ``dweight`` asked for; their share of the fp32 matrix peak
(157 TF) counts 2 * (present neighbours) * Cin * Cout FLOP.

``--model``: without a GPU -- the fp32 numpy model of the kernels' summation order (64-pair steps from zero, sequential add of the
steps, sequential add of the row chunks; the column sums in 16-row / 16-slot / 16-tile blocks) at the shapes
tests/test_gpu_sparse_conv_grad.py uses, as ratios to the BLAS-fp32 restatement's error; the timings are then "NOT MEASURED".
``--pairs LOG``: copy the accuracy pairs that test prints (lines starting with "sparse_conv bwd" / "sparse_conv train" / "sparse_conv
link") into the report.

Usage:  python tools/sparse_conv_bwd_time.py [--blocks 7] [--reps 10] [--model] [--pairs pytest.log] [--out profiles/sparse_conv_bwd.txt]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sparse_conv_time import B, N, PEAK_TF, VOXEL, alternate, block_us, offset_lists, room_points      # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- summation model
def _chain(A, Bm):
    """(p, M), (p, N): the sum over p of the outer products, one after the other in fp32, from zero."""
    acc = np.zeros((A.shape[1], Bm.shape[1]), np.float32)
    for p in range(A.shape[0]):
        acc = acc + np.outer(A[p], Bm[p]).astype(np.float32)
    return acc


def model_dweight(feats, gz, nbr, R):
    n_out, kvol = nbr.shape
    dw = np.zeros((kvol, feats.shape[1], gz.shape[1]), np.float32)
    for j in range(kvol):
        total = None
        for r0 in range(0, n_out, R):
            tot = np.zeros(dw.shape[1:], np.float32)
            for sub in range(r0, min(r0 + R, n_out), 1024):
                o = np.arange(sub, min(sub + 1024, r0 + R, n_out))
                o = o[nbr[o, j] >= 0]
                for p in range(0, len(o), 64):
                    tot = tot + _chain(feats[nbr[o[p:p + 64], j]], gz[o[p:p + 64]])
            total = tot if total is None else total + tot
        dw[j] = total
    return dw


def _slots16(rows):
    """16 slots stride over the rows, each a sequential sum; then the slots in ascending order."""
    slots = np.zeros((16, rows.shape[1]), np.float32)
    for s in range(16):
        for r in rows[s::16]:
            slots[s] = slots[s] + r
    acc = slots[0].copy()
    for s in range(1, 16):
        acc = acc + slots[s]
    return acc


def model_dbias(gz):
    return _slots16(np.stack([_slots16(gz[t:t + 256]) for t in range(0, gz.shape[0], 256)]))


def model_lines():
    from proxytransformation_amd import sparse
    from tests.sparse_util import host_map as _host_map, operands as _operands, rel as _rel, rows as _rows
    lines = ["fp32 numpy model of the kernels' summation order at the shapes of tests/test_gpu_sparse_conv_grad.py (CPU): error against the "
             "float64 restatement as a ratio to the BLAS-fp32 restatement's (the test's yardstick; the bar is 8)"]
    for cin, cout, k, s in [(64, 64, 3, 1), (64, 128, 3, 2), (128, 256, 1, 2)]:
        _, _, nbr = _host_map(4, k, s)
        ops = _operands(_rows(4)[0].shape[0], nbr.shape[0], cin, cout, k ** 3, seed=cin + cout)
        G = np.random.default_rng(cin).standard_normal((nbr.shape[0], cout)).astype(np.float32)
        r32 = sparse.sparse_conv3d_bwd_host(G, ops["feats"], nbr, ops["weight"], has_bias=True)
        r64 = sparse.sparse_conv3d_bwd_host(G.astype(np.float64), ops["feats"].astype(np.float64), nbr, ops["weight"].astype(np.float64), has_bias=True)
        R = 256                                              # what ptx_sparse_conv3d_bwd picks below ~ 1024 / tiles x 256 rows
        S = -(-nbr.shape[0] // R)
        yw, yb = _rel(r32["dweight"], r64["dweight"]), _rel(r32["dbias"], r64["dbias"])
        lines.append(f"  Cin={cin} Cout={cout} k={k} s={s} rows={nbr.shape[0]} ({S} chunks of {R}): dweight {_rel(model_dweight(ops['feats'], G, nbr, R), r64['dweight']) / yw:.2f} x "
                     f"(yardstick {yw:.2e});  dbias {_rel(model_dbias(G), r64['dbias']) / yb:.2f} x (yardstick {yb:.2e})")
    return lines


# ---------------------------------------------------------------------------------------------------------------- timing
def torch_layer(feats, weight, lists, n_out):
    out = torch.zeros((n_out, weight.shape[2]), dtype=torch.float32, device=feats.device)
    for j, (src, dst) in enumerate(lists):
        if src.numel():
            out = out.index_add(0, dst, feats.index_select(0, src) @ weight[j])
    return out


def layer_report(name, feats, kmap, weight, blocks, reps, lines, gen):
    from proxytransformation_amd import _abi, sparse
    lists = offset_lists(kmap.nbr)
    n_out, kvol = kmap.nbr.shape
    present = int((kmap.nbr >= 0).sum())
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    G = torch.randn((n_out, cout), generator=gen, device=feats.device)
    f, w = feats.clone().requires_grad_(), weight.clone().requires_grad_()

    def hip():
        return torch.autograd.grad(sparse.sparse_conv3d(f, kmap, w, differentiable=True), (f, w), G)

    def composed():
        return torch.autograd.grad(torch_layer(f, w, lists, n_out), (f, w), G)

    med, t, last = alternate({"hip": hip, "torch": composed}, blocks, reps)
    errs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(last["hip"], last["torch"])]
    lines.append(f"{name}: {feats.shape[0]} -> {n_out} rows, {kvol} offsets, {present} present neighbours ({present / max(n_out, 1):.1f} per row), "
                 f"Cin {cin}, Cout {cout}")
    lines.append(f"  forward + backward   hip {med['hip']:9.1f} us   torch {med['torch']:9.1f} us   ratio torch / hip = {med['torch'] / med['hip']:.2f}   "
                 f"max |hip - torch| / max |torch|: dfeats {errs[0]:.2e}, dweight {errs[1]:.2e}")
    if med["hip"] >= med["torch"]:
        lines.append("  NOTE: the HIP layer is NOT faster than the torch composition here.")
    # the dweight launches alone
    lib = _abi.lib()
    nbytes = lib.ptx_sparse_conv3d_bwd_workspace_bytes(n_out, kvol, cin, cout)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=feats.device)
    dw = torch.empty_like(weight)
    st = torch.cuda.current_stream(feats.device).cuda_stream

    def dweight_only():
        _abi.check(lib.ptx_sparse_conv3d_bwd(G.data_ptr(), None, None, 0, feats.data_ptr(), feats.shape[0], kmap.nbr.data_ptr(), None, n_out, kvol,
                                             weight.data_ptr(), cin, cout, None, None, None, None, dw.data_ptr(), ws.data_ptr(),
                                             ctypes.c_size_t(nbytes), st), "ptx_sparse_conv3d_bwd")
        return dw

    med_w, t_w, _ = alternate({"dweight": dweight_only}, blocks, reps)
    flop = 2.0 * present * cin * cout
    lines.append(f"  dweight launches alone {med_w['dweight']:9.1f} us   {flop / med_w['dweight'] * 1e-6:7.2f} TF = "
                 f"{100 * flop / med_w['dweight'] * 1e-6 / PEAK_TF:5.1f} % of the {PEAK_TF:g} TF fp32 matrix peak   (workspace {nbytes / 2 ** 20:.1f} MiB)")
    for k in ("hip", "torch"):
        lines.append(f"  {k} blocks (us): {[round(x, 1) for x in t[k]]}")
    lines.append(f"  dweight blocks (us): {[round(x, 1) for x in t_w['dweight']]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--pairs", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_conv_bwd.txt"))
    args = ap.parse_args()
    if not args.model and not torch.cuda.is_available():
        raise SystemExit("sparse_conv_bwd_time.py measures on a GPU: none found (--model runs the summation model on the CPU)")
    lines = []
    if torch.cuda.is_available():
        from bench import build_module
        from proxytransformation_amd import sparse
        from proxytransformation_amd.pipeline import level_coordinates
        from proxytransformation_amd.synth import CONFIGS
        device = torch.device("cuda:0")
        mod, _ = build_module(CONFIGS["cfg4_room"], device)
        gen = torch.Generator(device=device).manual_seed(7)
        lines.append(f"sparse convolution forward + backward on the voxel rows, {B} room clouds x {N} points at {VOXEL * 100:g} cm; "
                     f"{torch.cuda.get_device_name(0)}; median of {args.blocks} blocks of {args.reps} calls, sides alternating")
        rnd = lambda *shape: torch.randn(shape, generator=gen, device=device)          # noqa: E731
        with torch.no_grad():
            outs = [torch.from_numpy(room_points(900 + b, N)).to(device) for b in range(B)]
            coords, feats3, ends = mod.quantize(outs, VOXEL, return_scene_rows=True)
            c8, _, e8 = level_coordinates(coords, ends, 8, VOXEL)
            c64, _, e64 = level_coordinates(c8, e8, 64, VOXEL)
            maps = [("stem", feats3.contiguous(), sparse.kernel_map(coords, ends, 1, 3, 2), rnd(27, 3, 64) / 9.0),
                    ("64x64 at stride 8", rnd(c8.shape[0], 64), sparse.kernel_map(c8, e8, 8, 3, 1), rnd(27, 64, 64) / 41.6),
                    ("512x512 at stride 64", rnd(c64.shape[0], 512), sparse.kernel_map(c64, e64, 64, 3, 1), rnd(27, 512, 512) / 117.6)]
        for name, feats, kmap, weight in maps:
            layer_report(name, feats, kmap, weight, args.blocks, args.reps, lines, gen)
    else:
        lines.append("sparse convolution forward + backward: timings NOT MEASURED (no MI355X run; no speed claim is made)")
    if args.model:
        lines.append("")
        lines += model_lines()
    if args.pairs and os.path.exists(args.pairs):
        lines.append("")
        lines.append("accuracy pairs of tests/test_gpu_sparse_conv_grad.py: max |x - float64 reference| / max |reference| of the kernels (gpu) and of "
                     "the same fp32 chain on the CPU; the bar is gpu <= 8 x fp32-cpu")
        keep = ("sparse_conv bwd", "sparse_conv train", "sparse_conv link")
        lines += [ln[ln.index("sparse_conv "):].rstrip() for ln in open(args.pairs) if ln.lstrip(". ").startswith(keep)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
