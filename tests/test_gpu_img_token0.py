"""The mean token of AttentionPool2d as one more pixel (16-bit pooled path: csrc/api.hip run_img_proxy, `tok0`).

Token 0 is linear in the image mean, so the qkv0 launch produces q alone, the pooling pass takes s_h(0) from the head weights it
holds anyway (sum_c w_h(c) mean(c) + e_h(0)) and the o-projection's loader adds a_h(0) mean(f) to the pooled sums (T2m's column
in_dim carries the value row of the mean token).  These tests hold `img_proxy` -- through the stage API, like test_float_stages -- to
a float64 evaluation of the attention pool written here with torch on the CPU, from the same synthetic state dict, at the pooled
kernel's only shape (in_dim 512, 8 heads, C 256) with tile 1 holding 16 / 41 / 97 pixels and 1 / 3 / 33 images per call (33: a ragged
second 32-row tile in the qkv0 and o launches), bf16 and fp16 storage.

Inputs: the synthetic distribution of make_scene_batch; the same plus 10 sigma on every channel (the mean token then dominates the
score: s_h(0) and a_h(0) mean carry the result); images whose pixels all equal one vector (every pixel IS the mean, the softmax is
uniform up to the positional terms).

Bars: the project's (atol 5e-5, rtol 1e-5) on the synthetic inputs.  On the offset and constant inputs the parent commit's own maximum
error against the same reference on the same inputs was measured (profiles/img_token0_error.txt, PARENT_ERR below) and the new path
is held to twice that -- it re-orders fp32 sums the parent already rounds -- or to the project's bar where the parent is inside it.
"""
from functools import lru_cache
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import build_module

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HWS = (12, 13, 15)                  # image side: hw = 144 / 169 / 225 pixels
NIMG = (1, 3, 33)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
KINDS = ("synthetic", "offset", "constant")
ATOL, RTOL = 5e-5, 1e-5             # the project's bar for img_proxy (test_gpu_parity.py)
NMAX = max(NIMG)

#: the parent commit's max |img_proxy - float64 reference| over the three image sides and 33 images, per (kind, storage):
#: profiles/img_token0_error.txt.  All four are inside the project's bar (5e-5), so the bar alone decides today; the rule of twice
#: the parent's error is kept for an input class that leaves it.  (The new path on the same inputs: 2.170e-06, 2.369e-06,
#: 1.877e-06, 1.800e-06; the synthetic inputs: parent 1.363e-06 / 1.447e-06, new 1.380e-06 / 1.472e-06.)
PARENT_ERR = {
    ("offset", "bf16"): 2.170e-06, ("offset", "f16"): 2.369e-06,
    ("constant", "bf16"): 2.112e-06, ("constant", "f16"): 2.266e-06,
}


def _cfg(side, V=NMAX):
    from proxytransformation_amd.synth import PreshapeConfig
    return PreshapeConfig("tok0", B=1, N=2048, grid_size=4, dynamic_drop_radio=0.5, L=4, V=V, img_spacial_dim=side, seed_base=7100 + side)


@lru_cache(maxsize=None)
def _module(side):
    m, sd = build_module(_cfg(side))
    return m.cuda(), sd


@lru_cache(maxsize=None)
def features(side, kind, dt):
    """(33, in_dim, hw) features in the storage type `dt` (CPU tensor)."""
    from proxytransformation_amd.synth import make_scene_batch
    cfg = _cfg(side)
    img = torch.from_numpy(make_scene_batch(cfg)[3][0]).reshape(NMAX, cfg.input_dim, side * side)
    if kind == "offset":
        img = img + 10.0                                  # unit-variance channels: 10 sigma, common to every pixel
    elif kind == "constant":
        img = img[:, :, :1].expand(-1, -1, side * side).contiguous()
    return img.to(DTYPES[dt])


@lru_cache(maxsize=None)
def reference(side, kind, dt):
    """float64 img_proxy rows (33, C) of features(side, kind, dt): query = mean token, keys = mean token + pixels, positional terms,
    c_proj, norm_img (PRE:154-177, 335-342)."""
    _, sd = _module(side)
    w = {k: torch.from_numpy(np.asarray(v)).double() for k, v in sd.items() if k.startswith(("channel_mapper", "attn_pool2d", "norm_img"))}
    f = features(side, kind, dt).double()                                     # (n, in_dim, hw)
    C, heads = w["channel_mapper.weight"].shape[0], 8
    hd = C // heads
    x = f.transpose(1, 2) @ w["channel_mapper.weight"].reshape(C, -1).T + w["channel_mapper.bias"]      # (n, hw, C)
    x = torch.cat([x.mean(dim=1, keepdim=True), x], dim=1) + w["attn_pool2d.positional_embedding"][None]
    q = x[:, :1] @ w["attn_pool2d.q_proj.weight"].T + w["attn_pool2d.q_proj.bias"]
    k = x @ w["attn_pool2d.k_proj.weight"].T + w["attn_pool2d.k_proj.bias"]
    v = x @ w["attn_pool2d.v_proj.weight"].T + w["attn_pool2d.v_proj.bias"]
    n, T = x.shape[:2]
    q = q.reshape(n, 1, heads, hd).transpose(1, 2) * hd ** -0.5
    k = k.reshape(n, T, heads, hd).transpose(1, 2)
    v = v.reshape(n, T, heads, hd).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v                   # (n, heads, 1, hd)
    o = a.transpose(1, 2).reshape(n, C) @ w["attn_pool2d.c_proj.weight"].T + w["attn_pool2d.c_proj.bias"]
    mu = o.mean(dim=1, keepdim=True)
    var = ((o - mu) ** 2).mean(dim=1, keepdim=True)
    y = (o - mu) / torch.sqrt(var + 1e-5) * w["norm_img.weight"] + w["norm_img.bias"]
    return y.numpy()


@lru_cache(maxsize=None)
def _stages(side, nimg, dt):
    from tests.gpu_util import Stages
    m, _ = _module(side)
    assert abs(m.norm_img.eps - 1e-5) < 1e-12
    st = Stages(m, 1, 2048, 4, nimg)
    st.shape.img_dtype = {"bf16": 1, "f16": 2}[dt]       # the tables and the workspace do not depend on the storage type
    return st


def run(side, kind, dt, lo, hi):
    """img_proxy of images [lo, hi) of features(side, kind, dt) in one call -> (hi - lo, C) numpy."""
    img = features(side, kind, dt)[lo:hi].contiguous().cuda()
    out = _stages(side, hi - lo, dt).img_proxy(img)
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


def errors(side, kind, dt, nimg):
    """max |got - ref| and the largest excess over the project's bar (<= 0: inside it)."""
    got = run(side, kind, dt, 0, nimg).astype(np.float64)
    ref = reference(side, kind, dt)[:nimg]
    err = np.abs(got - ref)
    return float(err.max()), float((err - (ATOL + RTOL * np.abs(ref))).max())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("side", HWS)
def test_img_proxy_against_float64(side, dt):
    for kind in KINDS:
        for nimg in NIMG:
            worst, excess = errors(side, kind, dt, nimg)
            parent = PARENT_ERR.get((kind, dt))
            print(f"side {side} {dt} {kind} images {nimg}: max err {worst:.3e}, over the bar by {excess:.3e}, parent {parent}")
            if kind == "synthetic" or parent is None:
                assert excess <= 0.0, (side, dt, kind, nimg, worst)
            else:
                assert excess <= 0.0 or worst <= 2.0 * parent, (side, dt, kind, nimg, worst, parent)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("side", HWS)
def test_bit_identical_across_calls_and_batch_splits(side, dt):
    """Two calls on the same inputs agree bit for bit, and 33 images in one call equal the first 32 and the last one in calls of their
    own: no work-group reads k0 | v0, or rows next to its own, that nobody writes any more."""
    for kind in ("synthetic", "offset"):
        whole = run(side, kind, dt, 0, 33)
        assert np.array_equal(whole, run(side, kind, dt, 0, 33)), (side, dt, kind)
        parts = np.concatenate([run(side, kind, dt, 0, 32), run(side, kind, dt, 32, 33)])
        assert np.array_equal(whole, parts), (side, dt, kind)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_two_launch_form_of_the_table_product(dt):
    """From 4096 images per call on, q and [w_h | e_h] = q_h T1_h^T are two launches (the second reads q out of the 3 C-wide rows of
    the qkv0 buffer, whose k0 | v0 columns nobody writes on this path).  That size is the only way there: 4125 images -- the 33 of
    the other tests 125 times over -- held to the same float64 rows and the same bar."""
    side, reps = 12, 125
    for kind in ("synthetic", "offset"):
        img = features(side, kind, dt).repeat(reps, 1, 1).cuda()
        out = _stages(side, reps * NMAX, dt).img_proxy(img)
        torch.cuda.synchronize()
        got = out.cpu().numpy()[0].astype(np.float64)
        ref = np.tile(reference(side, kind, dt), (reps, 1))
        err = np.abs(got - ref)
        print(f"two-launch form, {dt} {kind}: max err {err.max():.3e}")
        assert (err <= ATOL + RTOL * np.abs(ref)).all(), (dt, kind, float(err.max()))


_LAYOUT_WORKER = r"""
import hashlib, sys, torch
sys.path.insert(0, %r)
from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
from tests.util import build_module
cfg = PreshapeConfig("tok0lay", B=2, N=8192, grid_size=8, dynamic_drop_radio=0.4, L=8, V=20, seed_base=7171)
m, _ = build_module(cfg)
m = m.cuda()
pts, text, mask, img = make_scene_batch(cfg)
dev = torch.device("cuda:0")
args = ([torch.from_numpy(p).to(dev) for p in pts],
        {"text_feats": torch.from_numpy(text).to(dev), "text_token_mask": torch.from_numpy(mask).to(dev)},
        torch.from_numpy(img).to(dev).to(torch.bfloat16))
with torch.no_grad():
    for _ in range(2):
        outs = m(*args)
    torch.cuda.synchronize()
m.check()
h = hashlib.sha256()
for o in outs:
    h.update(o.cpu().numpy().tobytes())
print("DIGEST", h.hexdigest(), [int(o.shape[0]) for o in outs])
"""


def test_forced_layouts_give_identical_outputs(tmp_path):
    """One small bf16 forward with PTX_LAYOUT forced both ways -- the clustering chain or the image chain on the caller's stream, the
    slot tags gated (k_select then has no completion event) or behind an event: the same bits."""
    script = tmp_path / "tok0_layout_worker.py"
    script.write_text(_LAYOUT_WORKER % ROOT)
    layouts = ("0--0", "0--1", "1---")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(os.environ, PTX_LAYOUT=lay), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for lay in layouts]
    digests = []
    for lay, p in zip(layouts, procs):
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, (lay, err[-2000:])
        digests.append([ln for ln in out.splitlines() if ln.startswith("DIGEST")][0])
    assert len(set(digests)) == 1, list(zip(layouts, digests))
