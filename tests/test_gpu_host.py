"""Host-side behaviour of the product module on the GPU: weight-change detection, independent library contexts
for concurrent module instances, the transform-returning forward, and the REAL module sharded over two ranks
(two processes sharing cuda:0, gloo) byte-for-byte against the unsharded run."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from proxytransformation_amd.synth import PreshapeConfig, fill_state_dict, make_scene_batch
from tests.util import build_module

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(cfg, scene_ids=None):
    from tests.gpu_util import t
    m, sd = build_module(cfg)
    pts, text, mask, img = make_scene_batch(cfg, scene_ids=scene_ids)
    return m.cuda(), sd, ([t(p) for p in pts], {"text_feats": t(text), "text_token_mask": t(mask)}, t(img))


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_every_kind_of_weight_change_is_picked_up():
    """The parameter-derived tables (folded BatchNorm, slot-bias tables, folded pooling matrices) must follow
    load_state_dict (copying and assign=True), re-assigned Parameters, optimiser-style in-place updates and --
    after invalidate_weights() or a train()/eval() switch -- writes through .data."""
    cfg = PreshapeConfig("w", B=2, N=3000, grid_size=4, dynamic_drop_radio=0.5, L=6, V=3, seed_base=71)
    m, sd, inp = _setup(cfg)
    base = [o.clone() for o in m(*inp)]
    alt = {k: torch.from_numpy(v).cuda() for k, v in fill_state_dict(m.state_dict(), salt=7).items()}

    def fresh(salt_sd):
        ref, _, _ = _setup(cfg)
        ref.load_state_dict(salt_sd)
        return [o.clone() for o in ref(*inp)]
    want_alt = fresh(alt)
    assert not _same(base, want_alt)
    m.load_state_dict(alt)                                   # in-place copy: versions bump
    assert _same(m(*inp), want_alt)
    orig = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    m.load_state_dict({k: v.clone() for k, v in orig.items()}, assign=True)   # new Parameter objects, old ones untouched
    assert _same(m(*inp), base)
    m.channel_mapper.weight = torch.nn.Parameter(alt["channel_mapper.weight"].clone())   # re-assigned Parameter
    mixed = dict(orig)
    mixed["channel_mapper.weight"] = alt["channel_mapper.weight"]
    want_mixed = fresh(mixed)
    assert _same(m(*inp), want_mixed)
    with torch.no_grad():                                    # optimiser-style in-place step
        m.channel_mapper.weight.copy_(orig["channel_mapper.weight"])
    assert _same(m(*inp), base)
    m.attn_pool2d.k_proj.weight.data.copy_(alt["attn_pool2d.k_proj.weight"])   # invisible to autograd ...
    m.eval()                                                 # ... until a mode switch (EMA hooks swap right before eval())
    mixed = dict(orig)
    mixed["attn_pool2d.k_proj.weight"] = alt["attn_pool2d.k_proj.weight"]
    assert _same(m(*inp), fresh(mixed))
    m.attn_pool2d.k_proj.weight.data.copy_(orig["attn_pool2d.k_proj.weight"])
    m.invalidate_weights()
    assert _same(m(*inp), base)


def test_two_modules_on_two_threads_do_not_share_events():
    """Each instance owns its side streams and fork / join events (PtxContext): two instances driven from two host
    threads on two torch streams of the same device give the results of running them one after the other."""
    cfgs = [PreshapeConfig("ta", B=3, N=9000, grid_size=5, dynamic_drop_radio=0.5, L=8, V=6, seed_base=81),
            PreshapeConfig("tb", B=2, N=7000, grid_size=4, dynamic_drop_radio=0.6, L=5, V=9, seed_base=82)]
    mods, inps, want = [], [], []
    for c in cfgs:
        m, _, inp = _setup(c)
        mods.append(m); inps.append(inp)
        want.append([o.clone() for o in m(*inp)])
    torch.cuda.synchronize()
    errs, got = [], [None, None]

    def worker(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(25):
                    outs = mods[i](*inps[i])
                st.synchronize()
                got[i] = [o.clone() for o in outs]
        except Exception as e:                               # pragma: no cover
            errs.append(repr(e))
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    torch.cuda.synchronize()
    assert not errs, errs
    for i in range(2):
        assert _same(got[i], want[i])


def test_forward_can_return_the_cluster_transforms():
    cfg = PreshapeConfig("rt", B=3, N=5000, grid_size=5, dynamic_drop_radio=0.5, L=7, V=4, seed_base=91)
    m, _, inp = _setup(cfg)
    d = m.forward_debug(*inp)
    outs, tf = m(*inp, return_transforms=True)
    torch.cuda.synchronize()
    assert _same(outs, d["outputs"])
    assert set(tf) == {"kcenter", "translate", "transform"}
    for k in tf:
        assert torch.equal(tf[k], d[k]), k
    assert tf["transform"].shape == (cfg.B, cfg.M_keep, 9)


_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from proxytransformation_amd.shard import ShardedPreshape
from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
from tests.util import build_module
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
dev = torch.device("cuda:0")
cfg = PreshapeConfig("sh", B=5, N=8000, grid_size=5, dynamic_drop_radio=0.5, L=9, V=7, seed_base=7300)
m, _ = build_module(cfg)
m = m.cuda()
sp = ShardedPreshape(m)
ids = sp.local_ids(cfg.B)
# every rank builds ONLY its own scenes (what a per-rank dataloader hands over)
pts, text, mask, img = make_scene_batch(cfg, scene_ids=ids)
t = lambda a: torch.from_numpy(a).to(dev)
lids, outs, allt = sp([t(p) for p in pts], {"text_feats": t(text), "text_token_mask": t(mask)}, t(img),
                      inputs="local", num_scenes=cfg.B, gather=True)
torch.cuda.synchronize()
assert lids == ids
torch.save(dict(ids=ids, outs=[o.cpu() for o in outs], allt=allt.cpu()), os.path.join(%r, f"rank{rank}.pt"))
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
'''


def test_real_module_sharded_over_two_ranks_matches_unsharded(tmp_path):
    cfg = PreshapeConfig("sh", B=5, N=8000, grid_size=5, dynamic_drop_radio=0.5, L=9, V=7, seed_base=7300)
    m, _, inp = _setup(cfg)
    outs, tf = m(*inp, return_transforms=True)
    torch.cuda.synchronize()
    want_t = torch.cat([tf["kcenter"], tf["translate"], tf["transform"]], -1).cpu()
    script = tmp_path / "w.py"
    script.write_text(_WORKER % (ROOT, str(tmp_path)))
    import socket
    with socket.socket() as sk:                 # a free port of this box, not a fixed one
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    for p in procs:
        out, _ = p.communicate(timeout=600)
        assert p.returncode == 0, out
    seen = set()
    for r in range(2):
        res = torch.load(tmp_path / f"rank{r}.pt")
        assert res["ids"] == list(range(r, cfg.B, 2))
        for sid, o in zip(res["ids"], res["outs"]):
            assert torch.equal(o, outs[sid].cpu()), f"scene {sid} differs between the sharded and the unsharded run"
            seen.add(sid)
        assert torch.equal(res["allt"], want_t), "gathered transforms differ"
    assert seen == set(range(cfg.B))


def test_forward_is_ordered_behind_in_place_input_writes():
    """The fork of the two chains (device-word gates, csrc/api.hip: the clustering stream waits for the first thread of the
    image chain's first kernel instead of an event) has to order the whole forward behind whatever the caller enqueued before
    it: the inputs are rewritten IN PLACE on the caller's stream right before every call, from three resident variants, and
    every output must equal the first pass over that variant bit for bit (a clustering stream that starts early, or reads
    stale lines, picks other clusters)."""
    # (a shape whose image chain is the longer one by the forward's estimate -- 40 + 0.18 B V > 80 + 0.42 Kd us -- so that the
    # image chain owns the caller's stream and the gates, not the events, order the chains)
    kw = dict(B=2, N=30000, grid_size=8, dynamic_drop_radio=0.4, L=16, V=180)
    cfg = PreshapeConfig("forksoak", seed_base=4242, **kw)
    assert 40 + 0.18 * cfg.B * cfg.V > 80 + 0.42 * cfg.Kd
    m, _ = build_module(cfg)
    m = m.cuda()
    dev = torch.device("cuda:0")
    variants = []
    for k in range(3):
        c = PreshapeConfig("forksoak", seed_base=4242 + 100 * k, **kw)
        pts, text, mask, img = make_scene_batch(c)
        variants.append(([torch.from_numpy(p).to(dev) for p in pts], torch.from_numpy(text).to(dev), torch.from_numpy(mask).to(dev),
                         torch.from_numpy(img).to(dev).to(torch.bfloat16)))
    pts = [p.clone() for p in variants[0][0]]
    td = {"text_feats": variants[0][1].clone(), "text_token_mask": variants[0][2].clone()}
    img = variants[0][3].clone()
    ref = {}
    with torch.no_grad():
        for i in range(90):
            key = (i * 7 + i // 5) % 3
            v = variants[key]
            for d, s_ in zip(pts, v[0]):
                d.copy_(s_)
            td["text_feats"].copy_(v[1]); td["text_token_mask"].copy_(v[2]); img.copy_(v[3])
            outs = m(pts, td, img)
            if key not in ref:
                ref[key] = [o.clone() for o in outs]
            else:
                assert len(outs) == len(ref[key])
                for a, b in zip(outs, ref[key]):
                    assert a.shape == b.shape and torch.equal(a, b), f"forward {i} (variant {key}) differs from the first pass"


def test_bench_multi_rank_path_on_one_gpu(tmp_path):
    """bench.py's own N > 1 path -- self-launch under torch.distributed.run, process-group init, barrier-bracketed timing,
    MAX all-reduce, the rank census -- exercised on the 1-GPU box: two ranks share cuda:0 over gloo (the numbers mean
    nothing; with --backend nccl the same code runs over RCCL on an 8-GPU node)."""
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    # (a) the reduced --full line, (b) the whole --full line: the extra legs
    # (fp32-stored features, bf16 compute) run on every rank behind real barriers, the rank-0-only reports are skipped
    for extra in (["--full", "--no-passes", "--no-cpu-baseline", "--time-every", "1"], ["--full", "--time-every", "1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                            "--steps", "2", "--warmup", "1", "--repeats", "2"] + extra,
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout                        # rank 0 prints ONE line
        d = json.loads(lines[0])
        assert d["n_gpus"] == 2 and d["config"]["global_scenes_per_step"] == 8 and d["config"]["scenes_per_gpu"] == 4
        assert d["cpu_baseline"] is None and d["value"] > 0 and d["scaling"] == "weak"
        assert [x[0] for x in d["ranks_seen"]] == [0, 1] and len({x[2] for x in d["ranks_seen"]}) == 2     # two processes
        assert d["roofline"]["launches"] == 4 and 0 < d["roofline"]["frac"] < 1          # 2 blocks x 2 steps, every launch timed
        tb = d["timed_blocks"]
        assert tb["blocks"] == 2 and len(tb["values"]) == 2 and tb["value_min"] <= d["value"] <= tb["value_max"]
        if "--no-passes" not in extra:
            assert d["value_f32_features"] > 0 and d["value_bf16_compute"] > 0 and "roofline_passes" not in d
    # (c) the plain line of `bench.py --gpus N` with --dump-outputs: one block, the headline alone, and both ranks writing their own
    # scenes into one directory.  Last timed step = step 1 -> input set 1 -> scenes (1 * 2 + rank) * 4 + b = 8..15.
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and [x[0] for x in d["ranks_seen"]] == [0, 1] and d["value"] > 0
    assert d["timed_blocks"]["blocks"] == 1 and d["timed_blocks"]["steps_per_block"] == 2
    assert d["roofline"] is None and d["cpu_baseline"] is None and not {"value_f32_features", "value_bf16_compute"} & set(d)
    assert sorted(os.listdir(out)) == [f"out_scene{s:05d}.npy" for s in range(8, 16)]
    arrs = [np.load(out / f"out_scene{s:05d}.npy") for s in range(8, 16)]
    assert all(a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3 and len(a) > 0 for a in arrs)


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    """The plain line `--gpus 1 --steps K --warmup W`: ONE block of exactly K timed steps and the headline alone (no roofline,
    CPU baseline or extra legs).  --dump-outputs writes what the last timed step returned -- step K - 1 of the rotation over
    three input sets -- the same bits on a second run, and the same as this process's own forward over those scenes."""
    import json
    from proxytransformation_amd.synth import CONFIGS
    steps, dumps = 5, []
    for run in range(2):
        out = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                            "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["unit"] == "scenes/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
        assert d["timed_blocks"]["blocks"] == 1 and d["timed_blocks"]["steps_per_block"] == steps
        assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 4e3 - 1) < 1e-3        # 4 scenes per step
        assert d["roofline"] is None and d["cpu_baseline"] is None
        assert not {"value_f32_features", "value_bf16_compute", "value_graph_replay", "train_step", "roofline_passes"} & set(d)
        ids = range(4, 8)                                   # step 4 -> input set 4 % 3 = 1 -> scenes 4..7
        assert sorted(os.listdir(out)) == [f"out_scene{s:05d}.npy" for s in ids]
        arrs = [np.load(out / f"out_scene{s:05d}.npy") for s in ids]
        assert all(a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3 for a in arrs)
        assert sum(a.nbytes for a in arrs) <= 64 << 20
        dumps.append(arrs)
    assert all(np.array_equal(a, b) for a, b in zip(*dumps))
    cfg = CONFIGS["cfg2"]
    m, _, (pts, td, img) = _setup(cfg, scene_ids=ids)
    with torch.no_grad():
        outs = m(pts, td, img.to(torch.bfloat16))
    assert all(np.array_equal(o.cpu().numpy(), a) for o, a in zip(outs, dumps[0]))


def test_bench_pipeline_plain_run_and_dumped_outputs(tmp_path):
    """`--pipeline` without --full: one timed block, no per-stage events / host-draw variant / CPU baseline.  --dump-outputs writes
    every output array of the last chained call (points, voxel rows, level points, sampled image features) within 64 MiB (a seeded
    sample of each array's rows once the cap applies), and the same files on a second run."""
    import json
    names, dumps = None, []
    for run in range(2):
        out = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cfg4_room", "--pipeline", "--steps", "2",
                            "--warmup", "1", "--dump-outputs", str(out)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        p = d["pipeline"]
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and len(p["ms_blocks"]) == 1 and d["cpu_baseline"] is None
        assert p["ms_per_stage"] is None and p["with_host_pixel_draws"] is None
        B = d["config"]["scenes_per_gpu"]
        names = ["coordinates", "features"] + [f"points_scene{b}" for b in range(B)] + \
            [f"level{li}_{k}_scene{b}" for li in range(4) for k in ("points", "imgfeats") for b in range(B)]
        assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
        arrs = {n: np.load(out / f"{n}.npy") for n in names}
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert arrs["coordinates"].dtype == np.float64 and np.array_equal(arrs["coordinates"], np.round(arrs["coordinates"]))
        assert all(a.dtype == np.float32 for n, a in arrs.items() if n != "coordinates")
        assert 0 < sum(len(arrs[f"points_scene{b}"]) for b in range(B)) <= p["surviving_points"]
        dumps.append(arrs)
    assert all(np.array_equal(dumps[0][n], dumps[1][n]) for n in names)


_NT_WORKER = r"""
import os, sys, hashlib, torch
sys.path.insert(0, %r)
from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
from tests.util import build_module
cfg = PreshapeConfig("ntstore", B=2, N=20000, grid_size=8, dynamic_drop_radio=0.5, L=16, V=24, seed_base=321)
m, _ = build_module(cfg)
m = m.cuda()
pts, text, mask, img = make_scene_batch(cfg)
dev = torch.device("cuda:0")
args = ([torch.from_numpy(p).to(dev) for p in pts],
        {"text_feats": torch.from_numpy(text).to(dev), "text_token_mask": torch.from_numpy(mask).to(dev)},
        torch.from_numpy(img).to(dev).to(torch.bfloat16))
with torch.no_grad():
    outs = m(*args)
h = hashlib.sha256()
for o in outs:
    h.update(o.cpu().numpy().tobytes())
print("DIGEST", h.hexdigest())
"""


@pytest.mark.gpu
def test_streaming_partial_stores_do_not_change_the_result(tmp_path):
    """k_img_pool stores its per-tile partials as plain or as streaming write-through lines depending on the image count of the
    launch (>= 4096 images: csrc/imgpool.hip); the switch is a cache policy, so both forms must give the same bits.  PTX_POOL_NT
    forces one or the other (read once per process: two processes)."""
    script = tmp_path / "nt_worker.py"
    script.write_text(_NT_WORKER % ROOT)
    digests = []
    for nt in ("0", "1"):
        env = dict(os.environ, PTX_POOL_NT=nt)
        r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        digests.append([ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0])
    assert digests[0] == digests[1]


def test_launch_count_of_the_benchmark_shape():
    """an eval forward at the benchmark's shape (bf16-stored features, head_dim 32) is 16 kernel launches (r02: 19; since r03 the two attention launches are one, and fc1 + fc2 + the output heads are one) --
    counted through the library's own launch-site bracketing (every launch of the forward sits in exactly one site)."""
    import ctypes
    from proxytransformation_amd import _abi
    from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
    from tests.util import build_module
    cfg = PreshapeConfig("launches", B=2, N=20000, grid_size=8, dynamic_drop_radio=0.5, L=16, V=20, seed_base=77)
    m, _ = build_module(cfg)
    m = m.cuda()
    pts, text, mask, img = make_scene_batch(cfg)
    dev = torch.device("cuda:0")
    args = ([torch.from_numpy(p).to(dev) for p in pts],
            {"text_feats": torch.from_numpy(text).to(dev), "text_token_mask": torch.from_numpy(mask).to(dev)},
            torch.from_numpy(img).to(dev).to(torch.bfloat16))
    lib = _abi.lib()
    nk = lib.ptx_kernel_count()
    with torch.no_grad():
        m(*args)                                    # tables, workspace
        torch.cuda.synchronize()
        lib.ptx_timing_select_mask((1 << nk) - 1)
        try:
            m(*args)
            torch.cuda.synchronize()
            n = (ctypes.c_int * nk)()
            ms = (ctypes.c_float * nk)()
            lib.ptx_timing_read_sites(n, ms, nk)
        finally:
            lib.ptx_timing_select(-1)
    per_site = {lib.ptx_kernel_name(i).decode(): n[i] for i in range(nk) if n[i]}
    assert sum(per_site.values()) == 16, per_site
    assert not any("k_gate" in k or "k_signal" in k for k in per_site), per_site      # clustering chain on the caller's stream: events


def test_launch_count_with_stream_gates():
    """The same count at a shape whose image chain owns the caller's stream (the benchmark's situation): the fork and the join are
    device-word gates there, and THEIR launches are counted too -- the 16 kernels + the fork's one-wave k_gate + the join's
    k_signal; the join's wait is folded into the proxy_proj GEMM (no k_gate launch on the caller's stream).  (One more where the
    attention runs as two launches.)"""
    import ctypes
    from proxytransformation_amd import _abi
    from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
    from tests.util import build_module
    cfg = PreshapeConfig("launches_g", B=2, N=20000, grid_size=8, dynamic_drop_radio=0.4, L=16, V=180, seed_base=78)
    assert 40 + 0.18 * cfg.B * cfg.V > 80 + 0.42 * cfg.Kd
    m, _ = build_module(cfg)
    m = m.cuda()
    pts, text, mask, img = make_scene_batch(cfg)
    dev = torch.device("cuda:0")
    args = ([torch.from_numpy(p).to(dev) for p in pts],
            {"text_feats": torch.from_numpy(text).to(dev), "text_token_mask": torch.from_numpy(mask).to(dev)},
            torch.from_numpy(img).to(dev).to(torch.bfloat16))
    lib = _abi.lib()
    nk = lib.ptx_kernel_count()
    with torch.no_grad():
        m(*args)
        torch.cuda.synchronize()
        if not m.uses_stream_gates():
            pytest.skip("this environment orders the streams with events (profiler / serialised queues / failed probe)")
        lib.ptx_timing_select_mask((1 << nk) - 1)
        try:
            m(*args)
            torch.cuda.synchronize()
            n = (ctypes.c_int * nk)()
            ms = (ctypes.c_float * nk)()
            lib.ptx_timing_read_sites(n, ms, nk)
        finally:
            lib.ptx_timing_select(-1)
    per_site = {lib.ptx_kernel_name(i).decode(): n[i] for i in range(nk) if n[i]}
    assert per_site.get("k_gate[fork]") == 1 and per_site.get("k_signal[join]") == 1 and "k_gate[join]" not in per_site, per_site
    assert per_site.get("k_minmax") == 1
    two_launch_attn = "k_attn32[proxy_as_key]" in per_site      # few (scene, head) pairs at this shape: PV through memory
    tags_off_chain = "k_gate[tags]" in per_site                 # the slot tags on the third stream: its one-wave gate + signal
    assert per_site.get("k_signal[tags]", 0) == int(tags_off_chain)
    assert sum(per_site.values()) == 16 + 2 + int(two_launch_attn) + 2 * int(tags_off_chain), per_site


_GATE_WORKER = r"""
import os, sys, hashlib, torch
sys.path.insert(0, %r)
if os.environ.get("GATE_TEST_LIBRARY") == "testhooks":          # read by THIS script, not by the package: the product has no such switch
    from proxytransformation_amd import _abi
    _abi.use_test_hooks_library()
from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
from tests.util import build_module
if os.environ.get("GATE_TEST_SHAPE", "image") == "cluster":      # the clustering chain owns the caller's stream ("cgate" words)
    cfg = PreshapeConfig("gatefault", B=2, N=30000, grid_size=8, dynamic_drop_radio=0.75, L=16, V=6, seed_base=4242)
else:
    cfg = PreshapeConfig("gatefault", B=2, N=30000, grid_size=8, dynamic_drop_radio=0.4, L=16, V=180, seed_base=4242)
m, _ = build_module(cfg)
m = m.cuda()
pts, text, mask, img = make_scene_batch(cfg)
dev = torch.device("cuda:0")
args = ([torch.from_numpy(p).to(dev) for p in pts],
        {"text_feats": torch.from_numpy(text).to(dev), "text_token_mask": torch.from_numpy(mask).to(dev)},
        torch.from_numpy(img).to(dev).to(torch.bfloat16))
mode = os.environ.get("GATE_TEST_MODE", "plain")
def digest(outs):
    h = hashlib.sha256()
    for o in outs:
        h.update(o.cpu().numpy().tobytes())
    return h.hexdigest()
with torch.no_grad():
    if mode == "stall":
        outs = m(*args)                                   # a clean first call: probe, tables
        torch.cuda.synchronize()
        print("GATES_BEFORE", m.uses_stream_gates())
        torch.cuda._sleep(int(2.0e9 * 0.9))              # ~0.5-0.9 s of work queued AHEAD of the forward on the caller's stream (the fork's bound is 6 x 30 ms)
    if mode in ("last-check", "last-exit", "last-del"):
        outs = m(*args)                                   # the ONLY forward: its join gate fails after the counts are out
        print("CALL", "ok")
        if mode == "last-check":
            try:
                m.check()
                print("CHECK", "silent")
            except RuntimeError as e:
                print("CHECK", "raised: " + str(e)[:160].replace("\n", " "))
            m.check()                                     # reported once
            print("CHECK2", "silent")
        elif mode == "last-del":
            import warnings, gc
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                del m, outs
                gc.collect()
            print("DEL", " | ".join(str(x.message)[:200].replace("\n", " ") for x in w))
        sys.stdout.flush()
        sys.exit(0)                                       # last-exit: the interpreter-exit hook must turn this into exit code 70
    calls = []
    for i in range(3):
        try:
            outs = m(*args)
            torch.cuda.synchronize()
            calls.append("ok nan=%%d" %% int(all(bool(torch.isnan(o).all()) for o in outs)))
        except RuntimeError as e:
            calls.append("raised: " + str(e)[:160].replace("\n", " "))
        if i == 0 and mode != "stall":
            print("GATES_BEFORE", m.uses_stream_gates() or "raised" in calls[0])
            print("GATE_BITS", m.stream_gate_bits())
    for c in calls:
        print("CALL", c)
    print("GATES_AFTER", m.uses_stream_gates())
    outs = m(*args)
    torch.cuda.synchronize()
    print("DIGEST", digest(outs))
"""


def _run_gate_worker(tmp_path, expect_rc=0, **env_extra):
    script = tmp_path / "gate_worker.py"
    script.write_text(_GATE_WORKER % ROOT)
    env = dict(os.environ, **env_extra)
    if "PTX_GATE_FAULT" in env_extra:       # the fault-injection hooks exist in the test-hooks build of the library only
        env["GATE_TEST_LIBRARY"] = "testhooks"
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == expect_rc, (r.returncode, r.stderr[-3000:])
    out = {"STDERR": [r.stderr]}
    for ln in r.stdout.splitlines():
        k, _, v = ln.partition(" ")
        out.setdefault(k, []).append(v)
    return out


@pytest.mark.parametrize("fault", ["fork", "join", "stall"])
def test_stream_gate_timeout_fails_loudly(tmp_path, fault):
    """A stream gate that runs out of time must not let go silently: the waiter stores an error word,
    the outputs of that forward become NaN, Python gets a RuntimeError -- from the same call when the fork fails (the error word is
    there before the survivor counts), from the next call when the join fails (the counts are published before the join) -- and
    the context then orders its streams with events and computes the right result again.  fork / join: the releasing store is
    dropped (PTX_GATE_FAULT); stall: nothing is injected, the caller's stream simply has more work queued ahead of the forward
    than the bound allows (PTX_GATE_TIMEOUT_MS = 30)."""
    ref = _run_gate_worker(tmp_path, PTX_GATE="0")                      # events from the start: the reference digest
    assert ref["GATES_AFTER"] == ["False"] and all(c == "ok nan=0" for c in ref["CALL"])
    env = dict(PTX_GATE_TIMEOUT_MS="30")
    if fault == "stall":
        env["GATE_TEST_MODE"] = "stall"
    else:
        env["PTX_GATE_FAULT"] = fault
    got = _run_gate_worker(tmp_path, **env)
    if got["GATES_BEFORE"] == ["False"]:
        pytest.skip("this environment orders the streams with events (profiler / serialised queues / failed probe)")
    calls = got["CALL"]
    if fault == "join":
        assert calls[0] == "ok nan=1", calls                            # returned (counts were out), outputs poisoned
        assert calls[1].startswith("raised:") and "stream gate timed out" in calls[1] and "join" in calls[1], calls
    else:
        assert calls[0].startswith("raised:") and "stream gate timed out" in calls[0] and "fork" in calls[0], calls
        assert calls[1] == "ok nan=0", calls
    assert calls[2] == "ok nan=0", calls
    assert got["GATES_AFTER"] == ["False"]                              # events from the failure on
    assert got["DIGEST"] == ref["DIGEST"]                               # and the result is right again


@pytest.mark.parametrize("how", ["check", "exit", "del"])
def test_join_failure_of_the_last_forward_is_not_lost(tmp_path, how):
    """VERDICT r04 #9 / ADVICE r04: a join gate fails AFTER the survivor counts are out, so forward() has already returned (NaN outputs);
    if that forward is the last one of a loop no later call reports it.  The module therefore keeps the lane marked unchecked:
    ``check()`` drains and raises once, garbage collection warns, and an interpreter that exits without either ends with exit
    code 70 and a message on stderr instead of 0."""
    probe = _run_gate_worker(tmp_path)
    if probe["GATES_BEFORE"] == ["False"]:
        pytest.skip("this environment orders the streams with events (profiler / serialised queues / failed probe)")
    env = dict(PTX_GATE_TIMEOUT_MS="30", PTX_GATE_FAULT="join", GATE_TEST_MODE="last-" + how)
    got = _run_gate_worker(tmp_path, expect_rc=70 if how == "exit" else 0, **env)
    assert got["CALL"] == ["ok"]
    if how == "check":
        assert got["CHECK"][0].startswith("raised:") and "stream gate timed out" in got["CHECK"][0] and "join" in got["CHECK"][0], got
        assert got["CHECK2"] == ["silent"]
    elif how == "del":
        assert "unreported failure" in got["DEL"][0] and "stream gate timed out" in got["DEL"][0], got
    else:
        assert "UNREPORTED FAILURE" in got["STDERR"][0] and "stream gate timed out" in got["STDERR"][0], got["STDERR"][0][-500:]


@pytest.mark.parametrize("fault", ["join", "tags", "join-early"])
def test_stream_gate_timeout_fails_loudly_on_the_clustering_layout(tmp_path, fault):
    """The same for the words of the layout in which the clustering chain owns the caller's stream (r04 "cgate": the wait for the
    image chain rides at the end of the qkv GEMM / of k_select, the wait for the slot tags at the end of the proj GEMM): a dropped
    releasing store gives NaN outputs, a RuntimeError naming the gate on the next call, events from then on, and the right result."""
    # join-early: the early-proxy form of the layout (forced at this small shape), where the join's wait is the end of k_select
    extra = dict(GATE_TEST_SHAPE="cluster", **({"PTX_LAYOUT": "-1--"} if fault == "join-early" else {}))
    fault = fault.split("-")[0]
    ref = _run_gate_worker(tmp_path, PTX_GATE="0", **extra)
    assert ref["GATES_AFTER"] == ["False"] and all(c == "ok nan=0" for c in ref["CALL"])
    got = _run_gate_worker(tmp_path, PTX_GATE_TIMEOUT_MS="30", PTX_GATE_FAULT=fault, **extra)
    clean = _run_gate_worker(tmp_path, **extra)                         # nothing injected: the gated layout gives the events' result
    assert all(c == "ok nan=0" for c in clean["CALL"]) and clean["DIGEST"] == ref["DIGEST"]
    if clean["GATE_BITS"] != ["3"]:
        pytest.skip("this environment orders the streams with events (profiler / serialised queues / failed probe)")
    calls = got["CALL"]
    if "PTX_LAYOUT" in extra:
        # the wait sits at the end of k_select, in front of the slot tags that publish the survivor counts: the error word is there
        # before the counts, so the SAME call raises (like a failed fork)
        assert calls[0].startswith("raised:") and "stream gate timed out" in calls[0] and "join" in calls[0], calls
        assert calls[1] == "ok nan=0", calls
    else:
        assert calls[0] == "ok nan=1", calls
        assert calls[1].startswith("raised:") and "stream gate timed out" in calls[1] and ("tags" if fault == "tags" else "join") in calls[1], calls
    assert calls[2] == "ok nan=0", calls
    assert got["GATES_AFTER"] == ["False"]
    assert got["DIGEST"] == ref["DIGEST"]



@pytest.mark.parametrize("shape", ["image-chain-long", "cluster-chain-long"])
def test_eval_forward_is_capturable_into_a_hip_graph(shape):
    """SURVEY 7.2 step 6 / VERDICT r03 missing #3: ``forward_padded`` (the eval forward without its host wait) captured with
    torch.cuda.graph and replayed on new input values written into the captured tensors -- both stream layouts of the forward (the
    image chain or the clustering chain on the caller's stream; inside a capture the two chains are ordered by events, which
    become graph edges) -- must give exactly what the eager forward gives on the same values, replay after replay (the
    workspace's clean-on-entry words are left clean by every forward, so a replay needs no clearing node)."""
    kw = dict(B=2, N=20000, grid_size=8, L=16, seed_base=6100)
    kw.update(dict(dynamic_drop_radio=0.4, V=180) if shape == "image-chain-long" else dict(dynamic_drop_radio=0.75, V=6))
    cfg = PreshapeConfig("graph", **kw)
    assert (40 + 0.18 * cfg.B * cfg.V > 80 + 0.42 * cfg.Kd) == (shape == "image-chain-long")
    m, _ = build_module(cfg)
    m = m.cuda()
    dev = torch.device("cuda:0")
    variants = []
    for k in range(3):
        c = PreshapeConfig("graph", **dict(kw, seed_base=6100 + 100 * k))
        pts, text, mask, img = make_scene_batch(c)
        variants.append(([torch.from_numpy(p).to(dev) for p in pts], torch.from_numpy(text).to(dev), torch.from_numpy(mask).to(dev),
                         torch.from_numpy(img).to(dev).to(torch.bfloat16)))
    pts = [p.clone() for p in variants[0][0]]
    td = {"text_feats": variants[0][1].clone(), "text_token_mask": variants[0][2].clone()}
    img = variants[0][3].clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):                                      # the lane of this stream: context, workspace, tables
            m.forward_padded(pts, td, img)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out_g, cnt_g = m.forward_padded(pts, td, img)
    for rep in range(6):
        v = variants[(rep * 2 + 1) % 3]
        for d, s_ in zip(pts, v[0]):
            d.copy_(s_)
        td["text_feats"].copy_(v[1]); td["text_token_mask"].copy_(v[2]); img.copy_(v[3])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = m(v[0], {"text_feats": v[1], "text_token_mask": v[2]}, v[3])        # eager, its own lane (default stream)
        torch.cuda.synchronize()
        n = cnt_g.cpu().tolist()
        assert n == [int(o.shape[0]) for o in want], (rep, n)
        for b, o in enumerate(want):
            assert torch.equal(out_g[b, : n[b]], o), f"replay {rep}, scene {b}"


def test_product_library_has_no_fault_injection_hook(tmp_path):
    """PTX_GATE_FAULT lives in the test-hooks build only (csrc/Makefile: libproxyt_hip_testhooks.so, -DPTX_TEST_HOOKS).
    With the PRODUCT library the variable is inert: the forward is right and nothing is reported."""
    script = tmp_path / "gate_worker.py"
    script.write_text(_GATE_WORKER % ROOT)
    env = dict(os.environ, PTX_GATE_FAULT="join", PTX_GATE_TIMEOUT_MS="30")
    env.pop("GATE_TEST_LIBRARY", None)
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    calls = [ln for ln in r.stdout.splitlines() if ln.startswith("CALL")]
    assert calls == ["CALL ok nan=0"] * 3, calls
    import re
    blob = open(os.path.join(ROOT, "proxytransformation_amd", "libproxyt_hip.so"), "rb").read()
    assert b"PTX_GATE_FAULT" not in blob and b"PTX_GATE_TRAP" not in blob
    # the whole switchboard of the product library (<= 12, each named in a test): PTX_GATE (events / gates:
    # test_stream_gate_timeout_fails_loudly), PTX_GATE_TIMEOUT_MS (same), PTX_LAYOUT (test_every_stream_layout_gives_the_same_result),
    # PTX_POOL_NT (test_streaming_partial_stores_do_not_change_the_result)
    names = sorted(set(m.decode() for m in re.findall(rb"PTX_[A-Z][A-Z_0-9]+", blob)))
    assert names == ["PTX_GATE", "PTX_GATE_TIMEOUT_MS", "PTX_LAYOUT", "PTX_POOL_NT"], names


_LAYOUT_WORKER = r"""
import os, sys, hashlib, torch
sys.path.insert(0, %r)
from proxytransformation_amd.synth import PreshapeConfig, make_scene_batch
from tests.util import build_module
which = os.environ["LAYOUT_SHAPE"]
if which == "cluster":       # 1 210 -> 691 kept clusters, 519 picks (the shipped gs = 12 grid) at a reduced N: the clustering chain is the long one
    cfg = PreshapeConfig("lay", B=3, N=30000, grid_size=12, dynamic_drop_radio=0.6, L=12, V=10, text_blocks=2, img_blocks=2, seed_base=4343)
else:                        # the benchmark's situation: the image chain is the long one
    cfg = PreshapeConfig("lay", B=2, N=30000, grid_size=8, dynamic_drop_radio=0.4, L=16, V=180, seed_base=4242)
m, _ = build_module(cfg)
m = m.cuda()
pts, text, mask, img = make_scene_batch(cfg)
dev = torch.device("cuda:0")
args = ([torch.from_numpy(p).to(dev) for p in pts],
        {"text_feats": torch.from_numpy(text).to(dev), "text_token_mask": torch.from_numpy(mask).to(dev)},
        torch.from_numpy(img).to(dev).to(torch.bfloat16 if which == "image" else torch.float32))
with torch.no_grad():
    for _ in range(3):
        outs = m(*args)
    torch.cuda.synchronize()
m.check()
h = hashlib.sha256()
for o in outs:
    h.update(o.cpu().numpy().tobytes())
print("DIGEST", h.hexdigest(), [int(o.shape[0]) for o in outs])
"""


@pytest.mark.parametrize("shape", ["image", "cluster"])
def test_every_stream_layout_gives_the_same_result(tmp_path, shape):
    """PTX_LAYOUT (csrc/api.hip) forces the per-shape layout decisions of the eval forward: which chain owns the caller's stream,
    early proxies, the image chain forked behind k_cluster, the slot tags behind a gate on the third stream.  Every forced
    arrangement -- with gates and with events -- must give what the rule's own choice gives.  (The early proxies re-associate a
    bias term, SURVEY H4-level rounding: they are compared among themselves and within 1e-5 of the rest.)"""
    script = tmp_path / "layout_worker.py"
    script.write_text(_LAYOUT_WORKER % ROOT)

    def run(**env_extra):
        env = dict(os.environ, LAYOUT_SHAPE=shape, **env_extra)
        r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, (env_extra, r.stderr[-2000:])
        return [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0]
    base = run()
    if shape == "image":
        for lay in ("0--0", "0--1", "1---", "10--"):
            for gate in ("0", "1"):
                assert run(PTX_LAYOUT=lay, PTX_GATE=gate) == base, (lay, gate)
        return
    # cluster shape: two families -- without and with the early proxies (the kept rows' qkv differ by fp32 rounding of the re-associated
    # bias term: same survivors, coordinates within the parity bar of each other; the rule picks the early form at this shape)
    plain = [run(PTX_LAYOUT=lay, PTX_GATE=gate) for lay in ("0---", "10--", "100-", "101-") for gate in ("0", "1")]
    early = [run(PTX_LAYOUT=lay, PTX_GATE=gate) for lay in ("11--", "110-", "111-") for gate in ("0", "1")]
    assert len(set(plain)) == 1, plain
    assert len(set(early)) == 1, early
    assert base in (plain[0], early[0])
    assert early[0].split(" ", 2)[2] == plain[0].split(" ", 2)[2]           # the same survivors per scene
