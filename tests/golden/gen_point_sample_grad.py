#!/usr/bin/env python3
"""Generate g7_point_sample_grad.npz: the gradient of the reference's own ``batch_point_sample`` with respect to the feature maps.

Runs ONLY where the reference checkout is present (like gen_golden.py, whose stand-ins for the framework imports are restated
here: its loader lives inside ``gen_point_sample``).  ``point_fusion.py`` is loaded by path, untouched, and run on the inputs
of g5_point_sample.npz -- its ``feats``, ``proj`` and the four cases' ``*_points`` / ``*_cfg`` -- with ``feats.requires_grad_()``;
a seeded standard-normal ``dout`` is backpropagated through torch's CPU autograd (F.grid_sample, the sum over the views, the
division).  The file holds ``<case>_dout`` (N, CH) and ``<case>_dfeats`` (V, CH, H, W) only.

The sampling treats every channel alike (the index of contributing (point, view) pairs is the same for all of them), so the
capture is taken on the first CH = 8 of g5's 32 channels: that keeps the file below the 1 MiB limit for committed files.

Usage:  python tests/golden/gen_point_sample_grad.py
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
REF = "/root/reference/embodiedscan"
CH = 8
CASES = ("plain", "aug", "flow3d", "bilinear")


def load_point_fusion():
    """point_fusion.py of the reference with the stand-ins of gen_golden (its registry, then those of gen_point_sample)."""
    from gen_golden import _install_standins
    _install_standins()
    mm = types.ModuleType("mmcv"); mmc = types.ModuleType("mmcv.cnn"); mmc.ConvModule = nn.Module
    me = types.ModuleType("mmengine"); mem = types.ModuleType("mmengine.model"); mem.BaseModule = nn.Module
    p3t = types.ModuleType("pytorch3d.transforms"); p3t.euler_angles_to_matrix = lambda *a, **k: None
    eu = types.ModuleType("embodiedscan.utils"); eu.ConfigType = dict
    sys.modules.update({"mmcv": mm, "mmcv.cnn": mmc, "mmengine": me, "mmengine.model": mem, "pytorch3d.transforms": p3t,
                        "embodiedscan.utils": eu})

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    load("embodiedscan.utils.array_converter", REF + "/utils/array_converter.py")
    b3 = load("embodiedscan.structures.bbox_3d", REF + "/structures/bbox_3d/utils.py")
    b3.get_proj_mat_by_coord_type = lambda *a, **k: None
    es_st = types.ModuleType("embodiedscan.structures"); es_st.__path__ = []
    sys.modules.setdefault("embodiedscan.structures", es_st)
    sys.modules["embodiedscan.structures.bbox_3d.utils"] = b3
    spec = importlib.util.spec_from_file_location("embodiedscan.structures.points", REF + "/structures/points/__init__.py",
                                                  submodule_search_locations=[REF + "/structures/points"])
    pts_mod = importlib.util.module_from_spec(spec)
    sys.modules["embodiedscan.structures.points"] = pts_mod
    spec.loader.exec_module(pts_mod)
    return load("pf_ref", REF + "/models/layers/fusion_layers/point_fusion.py")


def meta3d(g):
    """img_meta of the 'flow3d' case (tests/test_oracle_golden.py::_meta3d)."""
    return dict(transformation_3d_flow=["HF", "R", "S", "T"], pcd_horizontal_flip=True, pcd_vertical_flip=False,
                pcd_rotation=torch.from_numpy(g["flow3d_rot_T"]), pcd_scale_factor=float(g["flow3d_scale"]),
                pcd_trans=g["flow3d_trans"])


def main():
    torch.set_num_threads(1)
    pf = load_point_fusion()
    g = np.load(os.path.join(HERE, "g5_point_sample.npz"))
    rng = np.random.default_rng(7)
    save = {}
    for case in CASES:
        sx, sy, cw, ch, flip, ori_w = [float(x) for x in g[f"{case}_cfg"]]
        feats = torch.from_numpy(np.ascontiguousarray(g["feats"][:, :CH])).requires_grad_()
        pts = torch.from_numpy(g[f"{case}_points"])
        out = pf.batch_point_sample(meta3d(g) if case == "flow3d" else {}, img_features=feats, points=pts,
                                    proj_mat=torch.from_numpy(g["proj"]), coord_type="DEPTH",
                                    img_scale_factor=torch.tensor([sx, sy]), img_crop_offset=torch.tensor([cw, ch]),
                                    img_flip=bool(flip), img_pad_shape=(int(g["pad"][0]), int(g["pad"][1])),
                                    img_shape=(600, int(ori_w)), aligned=case == "bilinear")
        assert np.array_equal(out.detach().numpy(), g[f"{case}_out"][:, :CH]), case      # the forward of the g5 capture
        dout = rng.standard_normal(tuple(out.shape), dtype=np.float32)
        out.backward(torch.from_numpy(dout))
        dfeats = feats.grad.numpy()
        lhs = float((out.detach().double() * torch.from_numpy(dout).double()).sum())
        rhs = float((feats.detach().double() * feats.grad.double()).sum())
        print(f"g7_point_sample_grad/{case}: {len(pts)} points, nonzero pixels {(np.abs(dfeats).sum(1) > 0).mean():.3f}, "
              f"<out, dout> vs <feats, dfeats>: {abs(lhs - rhs) / abs(lhs):.1e} relative")
        save[f"{case}_dout"] = dout
        save[f"{case}_dfeats"] = dfeats
    path = os.path.join(HERE, "g7_point_sample_grad.npz")
    np.savez_compressed(path, **save)
    print(f"g7_point_sample_grad -> {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
