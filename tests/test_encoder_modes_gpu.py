"""Encoder host layer (csrc/bert_capi.hip): what a mode switch and a workspace regrowth must
leave behind, with graph replay on (rag_encoder_set_graphs(1), a side stream).

A captured graph holds the kernels of the mode it was captured under and the addresses of the
workspace it was captured in, so the setters and every regrowth drop the graphs:
  * after rag_encoder_set_defer_ln / rag_encoder_set_fusion the next forward of a shape that
    was captured before must run the NEW mode's kernels: its output equals, bit for bit, that of
    a fresh encoder (same weights) put into that mode before its first forward. A stale replay
    shows wherever the two modes' arithmetic differs, and the test checks that it does differ;
  * a batch that outgrows the token rows (first capacity 1024) and the CLS rows (256) regrows
    both groups; a small batch run before and after gives the same bits, and the large batch
    itself is right.
Oracle: bert_ref.bge_embed at test_encoder_graph_gpu.py's bar (5e-5). bge-small synthetic
weights, seed 11, fp16x3: their deferred-LayerNorm range bound is 19.9K (ragmi.encoders.
weight_bounds, host only), under the 60000 at which set_defer_ln(1) refuses with RAG_ERANGE,
so no step is skipped; the bound is asserted first.
"""
import numpy as np
import pytest
import torch

import bert_ref as R
from test_encoder_graph_gpu import _batch, _packed

pytestmark = pytest.mark.gpu

SEED = 11


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(R.BGE_SMALL, SEED)


def _encoder(weights, gpu, defer=-1, fusion=-1):
    from ragmi.encoders import HEAD_CLS_L2, BertEncoder
    enc = BertEncoder(R.BGE_SMALL, weights, HEAD_CLS_L2, gpu, "fp16x3")
    enc.set_graphs(1)
    enc.set_defer_ln(defer)
    enc.set_fusion(fusion)
    return enc


def _run(enc, packed, stream):
    with torch.cuda.stream(stream):
        out = enc.forward_packed(*packed)
    stream.synchronize()
    return out.cpu().numpy()


def test_mode_switch_drops_stale_graphs(weights, gpu):
    from ragmi.encoders import weight_bounds
    assert weight_bounds(R.BGE_SMALL, weights)[1] <= 60000.0     # set_defer_ln(1) is accepted
    bt = _batch(np.random.default_rng(3), 4, 8, 16)
    p = _packed(*bt)
    ref = R.bge_embed(weights, R.BGE_SMALL, *bt)
    st = torch.cuda.Stream(gpu)
    a = _encoder(weights, gpu)
    try:
        outs = [_run(a, p, st)]                                  # the shape's graph is captured
        assert np.abs(outs[0] - ref).max() <= 5e-5
        mode = {"defer": -1, "fusion": -1}
        for name, v in (("defer", 1), ("defer", 0), ("fusion", 1), ("fusion", -1)):
            (a.set_defer_ln if name == "defer" else a.set_fusion)(v)
            mode[name] = v
            got = _run(a, p, st)
            fresh = _encoder(weights, gpu, **mode)
            try:
                want = _run(fresh, p, st)
            finally:
                fresh.close()
            d = np.abs(got - ref).max()
            print(f"[{name}={v}] max|d| vs oracle {d:.3e}, bits changed by the switch: "
                  f"{int((got != outs[-1]).sum())}")
            assert np.array_equal(got, want), f"{name}={v}: not the fresh encoder's bits"
            assert d <= 5e-5
            outs.append(got)
        # the switches that change the arithmetic change bits: a stale replay could not hide
        assert not np.array_equal(outs[1], outs[0])             # deferred LayerNorm on
        assert not np.array_equal(outs[2], outs[1])             # ... and off again
        assert not np.array_equal(outs[3], outs[2])             # fused residual + LayerNorm on
        assert np.array_equal(outs[4], outs[2]) and np.array_equal(outs[2], outs[0])
    finally:
        a.close()


def test_regrowth_keeps_results(weights, gpu):
    rng = np.random.default_rng(4)
    small = _batch(rng, 2, 9, 11)                                # ~20 tokens
    large = _batch(rng, 300, 4, 6)                               # ~1500 tokens, 300 CLS rows
    assert int(large[2].sum()) > 1024 and large[2].shape[0] > 256
    st = torch.cuda.Stream(gpu)
    enc = _encoder(weights, gpu)
    try:
        x0 = _run(enc, _packed(*small), st)
        big = _run(enc, _packed(*large), st)
        x1 = _run(enc, _packed(*small), st)
        d = np.abs(big - R.bge_embed(weights, R.BGE_SMALL, *large))
        print(f"large batch: row 0 max|d| {d[0].max():.3e}, all rows {d.max():.3e}")
        assert np.array_equal(x1, x0)
        assert d[0].max() <= 5e-5
        assert np.abs(x0 - R.bge_embed(weights, R.BGE_SMALL, *small)).max() <= 5e-5
    finally:
        enc.close()
