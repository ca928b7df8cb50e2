"""The query selection, the decoder and the neck's head give the bits of the library before their kernels were folded onto shared pieces
(csrc/head.h): tests/golden/head_bits.json holds the SHA-256 of every output below as that library computed it.  All operands are
N(0, 1), so an order of addition shows in the bits; widths are 128 or 192 (two or three 64-wide blocks: the query selection adds per block
from zero, the decoder straight through), row counts cross a 64-row tile and leave a partial one."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from proxytransformation_amd import decoder, neck, query_select
from tests import decoder_util as du
from tests import query_select_util as qu
from tests import sparse_util as su

pytestmark = pytest.mark.gpu
DEV = su.DEV
GOLDEN = os.path.join(su.ROOT, "tests", "golden", "head_bits.json")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _digest(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def _posembed_module(cin, C, rng):
    """``PositionEmbeddingLearned`` in eval with N(0, 1) weights and running statistics off their initial values."""
    m = decoder._PositionEmbeddingLearned(cin, C)
    with torch.no_grad():
        for name, p in list(m.named_parameters()) + list(m.named_buffers()):
            if not p.is_floating_point():
                continue
            draw = rng.random(tuple(p.shape)) + 0.5 if name.endswith("running_var") else rng.standard_normal(tuple(p.shape))
            p.copy_(torch.from_numpy(draw.astype(np.float32)))
    return m.eval()


@functools.lru_cache(maxsize=None)
def outputs():
    """``{name: tensor}`` of every case, in one pass; the recorder of tests/golden/head_bits.json and the test below share it."""
    out = {}
    f = lambda rng, *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    with torch.no_grad():
        # the text score: rows (65, 1, 257), two token tiles
        feats, xyz, text, mask = qu.inputs(qu.SMALL_ROWS, 70, 128, 900)
        packed = query_select.pack([dev(a) for a in feats], [dev(p) for p in xyz], dev(mask))[0]
        bias = dev(f(np.random.default_rng(901), 1))
        out["score"] = query_select.score(packed, qu.SMALL_ROWS, dev(text), dev(mask), bias, scaled=True)

        # the regression branch's Linear: gathered through an index that crosses scenes inside a 64-row tile, then the rows themselves
        rng = np.random.default_rng(902)
        B, K, Lmax = 3, 40, 100
        index = dev(rng.integers(0, Lmax, (B, K)).astype(np.int64))
        h = query_select.linear(dev(f(rng, B, Lmax, 192)), dev(f(rng, 64, 192)), dev(f(rng, 64)), index, relu=True)
        out["qs_linear_gathered"] = h
        out["qs_linear_plain"] = query_select.linear(h, dev(f(rng, 128, 64)), dev(f(rng, 128)), None, relu=False)

        # the last Linear and the box decode behind the gathers
        rng = np.random.default_rng(903)
        x, coords = dev(f(rng, B, Lmax, 128)), dev((rng.integers(-500, 500, (B, Lmax, 3)) * 0.01).astype(np.float32))
        w, b, hid = dev(f(rng, 9, 128)), dev(f(rng, 9)), dev(f(rng, B, K, 128))
        for name, hh in (("decode_h", hid), ("decode_none", None)):
            q, qc, bx = query_select.decode(hh, w, b, x, coords, index)
            out[name + "_query"], out[name + "_coords"], out[name + "_boxes"] = q, qc, bx

        # the decoder's Linear: the fused add below add_cols, bias, ReLU, residual
        rng = np.random.default_rng(904)
        out["dec_linear"] = decoder.linear(dev(f(rng, 130, 192)), dev(f(rng, 128, 192)), dev(f(rng, 128)), add=dev(f(rng, 130, 192)),
                                           relu=True, add_cols=64, residual=dev(f(rng, 130, 128)))

        for cin in (3, 9):
            rng = np.random.default_rng(905 + cin)
            out[f"posembed_{cin}"] = decoder.posembed(dev(f(rng, 1, 130, cin)), _posembed_module(cin, 128, rng))

        # attention: a fully masked 64-key tile in scene 0, scattered masked keys in scene 1
        for heads in (4, 2):
            rng = np.random.default_rng(920 + heads)
            m = np.zeros((2, 130), bool)
            m[0, 64:128] = True
            m[1] = rng.random(130) < 0.3
            out[f"attention_hd{128 // heads}"] = decoder.attention(dev(f(rng, 2, 65, 128)), dev(f(rng, 2, 130, 128)),
                                                                   dev(f(rng, 2, 130, 128)), dev(m), heads)

        rng = np.random.default_rng(930)
        out["ln_first"], out["ln_second"] = decoder.layer_norm(dev(f(rng, 17, 128)), (dev(f(rng, 128)), dev(f(rng, 128))),
                                                               (dev(f(rng, 128)), dev(f(rng, 128))))

        rng = np.random.default_rng(931)
        out["boxes"] = decoder.boxes(dev(f(rng, 130, 128)), dev(f(rng, 9, 128)), dev(f(rng, 9)), dev(f(rng, 130, 3)))

        rng = np.random.default_rng(932)
        out["contrastive_scores"] = decoder.contrastive_scores(dev(f(rng, 2, 2, 65, 128)), dev(f(rng, 2, 70, 128)), dev(qu.text_mask(2, 70, 933)),
                                                               dev(f(rng, 1)), scaled=True, max_text_len=80)

        rng = np.random.default_rng(934)
        out["neck_head_cls"], out["neck_head_score"] = neck.neck_head(dev(f(rng, 17, 128)), dev(f(rng, 1, 128, 3)), dev(f(rng, 3)))

        # end to end: QuerySelect, the decoder behind it, the head scores
        feats, xyz, text, mask = qu.e2e_inputs()
        qs, dec = du.e2e_modules()
        qs, dec = qs.to(DEV), dec.to(DEV)
        keep = {}
        d, head = qs([dev(a) for a in feats], None, [dev(p) for p in xyz], dev(text), dev(mask), keep_out=keep)
        hs, bx = dec(query=d["query"], key=d["feats"], value=d["feats"], key_padding_mask=d["feats_attention_mask"], self_attn_mask=None,
                     cross_attn_mask=None, query_coords=d["query_coords"], key_coords=d["feats_coords"], pred_bboxes=d["pred_bboxes"],
                     text_feats=d["text_feats"], text_attention_mask=d["text_attention_mask"], bbox_head=qs)
        out.update(e2e_hidden=hs, e2e_boxes=bx, e2e_scores=dec.head_scores(hs, head, qs), e2e_index=keep["index"])
        torch.cuda.synchronize()
    return out


def digests():
    return {k: _digest(v) for k, v in outputs().items()}


def test_every_output_is_the_parent_commits_bits():
    """24 outputs: the score, both Linears of the query selection, the decode with and without ``h``, the decoder's Linear, both position
    embeddings, the attention at both head dimensions, both LayerNorm results, the boxes, the contrastive scores, the neck's head and the
    end-to-end case.  The top-k kernels have no digest: their own tests compare indices bit for bit with the host."""
    got = digests()
    print(json.dumps(got))
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    differ = [k for k in got if got[k] != want[k]]
    assert not differ, f"{len(differ)} of {len(got)} outputs differ: {differ}"
