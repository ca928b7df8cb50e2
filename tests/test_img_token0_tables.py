"""Host-side check (no GPU) of the algebra behind the q-only qkv0 launch: from the float64 weights, the q rows of W3 / b3, column
in_dim of T1 and of T2m (csrc/prep.hip) and the two identities

    scale q_h . k0_h                      = sum_c w_h(c) mean(c) + e_h(0)
    a_h(0) v0_h + sum_p a_h(p) v_h(p)     = [g_h + a_h(0) mean | a_h(0), a_h(1..hw)] T2m_h^T

reproduce q . k0 and v0 of the reference formula (token 0 = channel_mapper(mean) + pos_0 through k_proj / v_proj) to float64
rounding.  (k_proj's bias shifts every score of a head alike and v_proj's bias is the o-projection's bias: neither is in a table.)"""
import numpy as np
import pytest

from proxytransformation_amd import MODELS
from proxytransformation_amd.synth import PreshapeConfig, fill_state_dict


@pytest.mark.parametrize("side", [12, 15])
def test_token0_tables_reproduce_k0_and_v0(side):
    cfg = PreshapeConfig("tok0", B=1, N=1024, grid_size=4, dynamic_drop_radio=0.5, L=4, V=2, img_spacial_dim=side)
    m = MODELS.build(dict(type="ProxyTransformationNormReverse", **cfg.module_kwargs()))
    sd = {k: np.asarray(v, np.float64) for k, v in fill_state_dict(m.state_dict()).items()}
    C, in_dim, heads, hw = cfg.embed_dim, cfg.input_dim, cfg.num_heads, side * side
    hd, scale = C // heads, (C // heads) ** -0.5
    Wc, bc = sd["channel_mapper.weight"].reshape(C, in_dim), sd["channel_mapper.bias"]
    pos = sd["attn_pool2d.positional_embedding"]
    Wq, bq = sd["attn_pool2d.q_proj.weight"], sd["attn_pool2d.q_proj.bias"]
    Wk, Wv = sd["attn_pool2d.k_proj.weight"], sd["attn_pool2d.v_proj.weight"]
    assert pos.shape == (hw + 1, C)

    # the tables as prep.hip builds them
    W3q, b3q = Wq @ Wc, Wq @ (bc + pos[0]) + bq
    T1 = scale * np.concatenate([Wk @ Wc, Wk @ (bc[None] + pos).T], axis=1)          # (C, in_dim + hw + 1): column in_dim + i = token i
    T2m = np.concatenate([Wv @ Wc, Wv @ (bc[None] + pos).T], axis=1)                 # (C, in_dim + hw + 1)

    rng = np.random.default_rng(5)
    f = rng.standard_normal((in_dim, hw)) + 3.0                                      # one image, off zero mean
    mean = f.mean(axis=1)
    # the reference formula
    x = np.concatenate([(Wc @ mean + bc)[None], (Wc @ f).T + bc], axis=0) + pos     # (hw + 1, C) tokens
    q = Wq @ x[0] + bq
    k, v = x @ Wk.T, x @ Wv.T                                                        # (hw + 1, C), biases left out (docstring)
    assert np.allclose(W3q @ mean + b3q, q, rtol=1e-12, atol=1e-12)
    for h in range(heads):
        sl = slice(h * hd, (h + 1) * hd)
        we = q[sl] @ T1[sl]                                                          # [w_h | e_h], (in_dim + hw + 1)
        s_ref = scale * (k[:, sl] @ q[sl])                                           # every token's score
        s0 = we[:in_dim] @ mean + we[in_dim]
        assert abs(s0 - s_ref[0]) <= 1e-11 * max(1.0, abs(s_ref[0]))
        assert np.allclose(we[:in_dim] @ f + we[in_dim + 1:], s_ref[1:], rtol=1e-11, atol=1e-11)
        v0 = T2m[sl, :in_dim] @ mean + T2m[sl, in_dim]
        assert np.allclose(v0, v[0, sl], rtol=1e-11, atol=1e-11)
        a = np.exp(s_ref - s_ref.max())
        a /= a.sum()
        g = f @ a[1:]                                                                # sum_p a_h(p) f(., p)
        merged = np.concatenate([g + a[0] * mean, a]) @ T2m[sl].T
        assert np.allclose(merged, a @ v[:, sl], rtol=1e-11, atol=1e-11)
