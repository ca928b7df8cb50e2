"""CPU checks of the device sampler of the multi-view ingest (``MultiViewIngest(sampler="device")``, ``ptx_ingest_draw``): the C-ABI
surface and its argument checks (no kernel is enqueued), and the sampling properties of ``ingest.device_choices`` -- the exact host
restatement of the kernel's draws, which the GPU tests pin the kernel to bit for bit.  Every key is fixed: the tests are
deterministic."""
import ctypes
import os

import numpy as np
import pytest

from proxytransformation_amd import _abi
from proxytransformation_amd.ingest import MultiViewIngest, device_choices, scene_key
from tests.util import header_prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTX_EINVAL = -1


def _spearman(x):
    """Spearman rho of (position, value) for a sequence of distinct values."""
    r = np.empty(len(x))
    r[np.argsort(x)] = np.arange(len(x))
    p = np.arange(len(x), dtype=np.float64)
    return float(np.corrcoef(p, r)[0, 1])


def _chi2(counts, expected):
    counts = np.asarray(counts, np.float64)
    return float(((counts - expected) ** 2 / expected).sum())


def test_header_declares_and_library_exports_the_draw():
    src = open(os.path.join(ROOT, "include", "proxyt.h")).read()
    assert header_prototypes()["ptx_ingest_draw"][0] == "int"
    assert "#define PTX_ABI_VERSION 13" in src and _abi.ABI_VERSION == 13
    assert "ptx_ingest_draw" in _abi.SIGNATURES
    lib = _abi.lib()
    assert lib.ptx_abi_version() == _abi.ABI_VERSION
    getattr(lib, "ptx_ingest_draw")


@pytest.mark.parametrize("bad", ["null_ws", "null_sel", "null_status", "V0", "H0", "per_view0", "N0", "too_many_views"])
def test_draw_rejects_bad_arguments_before_any_enqueue(bad):
    """Every check is on the host and returns PTX_EINVAL with a message; the pointers are never touched (they are bogus here)."""
    lib = _abi.lib()
    args = dict(V=4, H=8, W=8, per_view=10, N=100, key=1, ws=0x1000, ws_bytes=1 << 20, sel=0x2000, status=0x3000)
    upd = {"null_ws": dict(ws=None), "null_sel": dict(sel=None), "null_status": dict(status=None), "V0": dict(V=0),
           "H0": dict(H=0), "per_view0": dict(per_view=0), "N0": dict(N=-1), "too_many_views": dict(V=4097)}[bad]
    args.update(upd)
    rc = lib.ptx_ingest_draw(args["V"], args["H"], args["W"], args["per_view"], args["N"], args["key"], args["ws"], args["ws_bytes"],
                             args["sel"], args["status"], None)
    assert rc == PTX_EINVAL
    msg = lib.ptx_last_error().decode()
    assert msg.startswith("ptx_ingest_draw:"), msg


def test_sampler_argument():
    with pytest.raises(ValueError):
        MultiViewIngest(1000, sampler="gpu")
    assert MultiViewIngest(1000).sampler == "host"                       # the default stays the numpy path
    assert MultiViewIngest(1000, sampler="device").sampler == "device"


def test_without_replacement_distinct_and_in_range():
    vc = [3000, 0, 500, 7000, 1, 0, 499]
    per_view, n = 500, 1200
    sel, stages = device_choices(vc, per_view, n, key=11, return_stages=True)
    assert sel.dtype == np.int64 and sel.shape == (n,)
    ne = [c for c in vc if c > 0]
    assert len(stages) == len(ne) + 1                                    # one draw per NON-EMPTY view, then the scene's
    for c, st in zip(ne, stages[:-1]):
        assert st.shape == (per_view,) and st.min() >= 0 and st.max() < c
        if c >= per_view:
            assert len(np.unique(st)) == per_view                         # without replacement
    assert stages[3].shape == (per_view,) and (stages[3] == 0).all()     # the 1-pixel view: with replacement, one value
    q = stages[-1]
    T = len(ne) * per_view
    assert T >= n and len(np.unique(q)) == n and q.min() >= 0 and q.max() < T
    assert sel.min() >= 0 and sel.max() < sum(vc)
    # cnt == per_view: a permutation of the whole view
    _, st2 = device_choices([50, 80], 50, 60, key=3, return_stages=True)
    assert sorted(st2[0].tolist()) == list(range(50))


def test_replacement_exactly_when_too_few():
    # per view: cnt < per_view -> repeats; cnt >= per_view -> none
    _, st = device_choices([40, 41, 39, 1000], 40, 100, key=5, return_stages=True)
    assert len(np.unique(st[0])) == 40 and len(np.unique(st[1])) == 40 and len(np.unique(st[3])) == 40
    assert len(np.unique(st[2])) < 40 and st[2].max() < 39
    # the aggregate: E * per_view < N -> with replacement (repeats, every position < T); == N -> a permutation of all
    _, st = device_choices([100, 0, 100], 30, 61, key=6, return_stages=True)
    assert len(np.unique(st[-1])) < 61 and st[-1].max() < 60
    _, st = device_choices([100, 0, 100], 30, 60, key=6, return_stages=True)
    assert sorted(st[-1].tolist()) == list(range(60))


def test_empty_views_contribute_nothing():
    vc = [0, 2000, 0, 0, 3000, 0]
    sel, st = device_choices(vc, 100, 150, key=21, return_stages=True)
    assert len(st) == 3
    off = np.cumsum([0] + vc)
    view_of = np.searchsorted(off, sel, side="right") - 1
    assert set(view_of.tolist()) <= {1, 4}
    # the draws are keyed by the view's index: empty views appended at the end change nothing
    assert np.array_equal(device_choices(vc + [0, 0], 100, 150, key=21), sel)
    with pytest.raises(ValueError):
        device_choices([0, 0, 0], 10, 5, key=1)


def test_inclusion_is_uniform():
    """Chi-square over many keys at a small m, for both stages and both modes (9 degrees of freedom: 99.999 % quantile ~ 37)."""
    m, keys = 10, range(2000)
    per_view_counts = np.zeros(m)
    agg_counts = np.zeros(m)
    repl_counts = np.zeros(m)
    for k in keys:
        # per view: 3 of 10 without replacement; the aggregate: 1 view x 10 draws -> 4 positions out of 10 without replacement
        sel, st = device_choices([m], 10, 4, key=k, return_stages=True)
        agg_counts += np.bincount(st[-1], minlength=m)
        _, st3 = device_choices([m, m, m, m], 3, 1, key=k, return_stages=True)
        per_view_counts += np.bincount(st3[1], minlength=m)
        _, str_ = device_choices([m], 25, 1, key=k, return_stages=True)             # with replacement: 25 from 10
        repl_counts += np.bincount(str_[0], minlength=m)
    assert _chi2(agg_counts, 2000 * 4 / m) < 37, agg_counts
    assert _chi2(per_view_counts, 2000 * 3 / m) < 37, per_view_counts
    assert _chi2(repl_counts, 2000 * 25 / m) < 37, repl_counts


def test_output_order_is_random():
    """Not sorted: the value is uncorrelated with its position (mean Spearman rho ~ 0) and the first element is uniform."""
    rhos = []
    firsts = np.zeros(16)
    for k in range(300):
        _, st = device_choices([1000], 1000, 1000, key=1000 + k, return_stages=True)
        rhos.append(_spearman(st[-1]))
        rhos.append(_spearman(st[0]))
    for k in range(3200):
        _, st = device_choices([16], 16, 16, key=k, return_stages=True)
        firsts[st[0][0]] += 1
    # one rho of a random permutation of 1000 has sd 1 / sqrt(999); the mean of 600 of them 5 sd from 0
    assert abs(np.mean(rhos)) < 5 / np.sqrt(999) / np.sqrt(len(rhos)), np.mean(rhos)
    assert max(abs(r) for r in rhos) < 0.2
    assert _chi2(firsts, 3200 / 16) < 60, firsts                                  # 15 dof: 99.999 % quantile ~ 48


def test_view_shares_of_the_aggregate():
    vc = [5000, 0, 300, 8000, 0, 1200, 2600, 40, 9000, 700]               # two views with fewer pixels than per_view
    per_view, n = 1000, 5000
    ne = [v for v, c in enumerate(vc) if c > 0]
    off = np.cumsum([0] + vc)
    E = len(ne)
    p = 1.0 / E
    sd = np.sqrt(n * p * (1 - p))                                          # binomial bound of the hypergeometric spread
    for key in (1, 2, 3):
        sel = device_choices(vc, per_view, n, key=key)
        view_of = np.searchsorted(off, sel, side="right") - 1
        share = np.bincount(view_of, minlength=len(vc))
        for v in ne:
            assert abs(share[v] - n / E) < 5 * sd, (key, v, share[v])
        assert share[[v for v in range(len(vc)) if v not in ne]].sum() == 0


def test_keys_decide_the_draw():
    vc = [3000, 0, 500, 7000]
    a = device_choices(vc, 400, 1000, key=77)
    assert np.array_equal(a, device_choices(vc, 400, 1000, key=77))
    assert np.array_equal(a, device_choices(vc, 400, 1000, key=77 + (1 << 64)))    # a 64-bit key
    b = device_choices(vc, 400, 1000, key=78)
    assert not np.array_equal(a, b) and (a != b).mean() > 0.9
    # per-scene keys of one call: a splitmix64 stream, distinct per position, fixed per (seed, position)
    ks = [scene_key(123, b) for b in range(6)]
    assert len(set(ks)) == 6 and ks == [scene_key(123, b) for b in range(6)] and ks != [scene_key(124, b) for b in range(6)]
    assert all(0 <= k < (1 << 64) for k in ks)
