"""Two pieces of work the ragged fp32 encoder leaves out on its un-split form (csrc/encoder.hip, include/gdr_hip.h), both exact:

* the token table: block 0's q/k/v depend on the token id alone (T5 adds no position embedding, modeling_t5.py:725; the norm is
  per row, :164-171; rows of a linear are independent), so a [vocab, 3*inner] table made with the encoder's own norm and linear is
  gathered instead of computed;
* a pooled-only call needs the last block's q for the B CLS rows alone (main_models.py:102-109 reads h[:,0]): k and v run over
  every live row, q over B rows (GDR_ENC_LAST_Q_CLS, read once per process, hence child processes).

Every comparison is torch.equal / a digest: nothing here may change a bit.  The padded form (gdr_t5_encoder_forward), which never
reads the table, is the independent computation.  Base width with two blocks and a 1000-row vocabulary (not a multiple of the
128-row tile: the table's last row panel is partial); (100, 40) and (130, 33) are the smallest batches on the un-split form,
(64, 40) is on the split forms, which must not change."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gdr_amd import synth
from gdr_amd.config import GDRConfig

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = 1000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def encs(dev):
    from gdr_amd import ops
    cfg = GDRConfig.base(vocab_size=VOCAB, num_layers=2)
    sd = synth.make_state_dict(cfg, seed=99, with_decoder=False)
    return cfg, ops.T5EncoderHandle(cfg, sd, dev, token_table=True), ops.T5EncoderHandle(cfg, sd, dev, token_table=False)


def _batch(B, L):
    """Ragged batch with the rows that take their own paths: fully masked, a hole, one token; ids 0 and VOCAB - 1; one id in
    several sequences."""
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=VOCAB, seed=3 + B, min_len=8)
    mask[3] = 0                                               # fully masked: keeps all L rows
    mask[7] = 1
    mask[7, 10:14] = 0                                        # hole: keeps all L rows
    mask[13] = 0
    mask[13, 0] = 1                                           # a single token
    ids[0, 0], ids[1, 0], ids[13, 0] = 0, VOCAB - 1, VOCAB - 1
    ids[2, 1] = ids[4, 1] = ids[5, 2] = ids[7, 12] = 77       # live positions (lengths are >= 8), and one under the hole
    return ids, mask


def _kept(mask):
    m = np.asarray(mask) != 0
    keep = np.ones(m.shape, bool)
    for b in range(m.shape[0]):
        n = int(m[b].sum())
        if n > 0 and m[b, :n].all():
            keep[b, n:] = False
    return keep


def test_handle_reports_the_table(encs):
    cfg, enc_t, enc_n = encs
    inner = cfg.num_heads * cfg.d_kv
    assert enc_t.token_table.shape == (VOCAB, 3 * inner) and enc_t.token_table_bytes == VOCAB * 3 * inner * 4
    assert enc_t.struct.qkv0_table == enc_t.token_table.data_ptr()
    assert enc_n.token_table is None and enc_n.token_table_bytes == 0 and not enc_n.struct.qkv0_table


@pytest.mark.parametrize("n", [37, 300])
def test_table_rows_are_the_encoders_own_values(dev, encs, n):
    """table[id] == linear(t5_layer_norm(embed[id]), wqkv0) bit for bit, for a row count inside one 64-row tile and one over several;
    the table itself was made in one 1000-row launch (its last row panel partial)."""
    from gdr_amd import ops
    cfg, enc_t, _ = encs
    g = np.random.Generator(np.random.PCG64(n))
    ids = g.integers(0, VOCAB, size=n)
    ids[:5] = [0, VOCAB - 1, 0, 511, 511]
    it = torch.from_numpy(ids).to(dev)
    want = ops.linear(ops.t5_layer_norm(enc_t.embed[it], enc_t._ln0, cfg.layer_norm_epsilon), enc_t._wqkv0)
    assert torch.equal(enc_t.token_table[it], want)


def test_refresh_rebuilds_the_table(encs):
    _, enc_t, _ = encs
    before = enc_t.token_table.clone()
    enc_t.token_table.zero_()
    assert enc_t.refresh_token_table() is enc_t and torch.equal(enc_t.token_table, before)


@pytest.mark.parametrize("B,L", [(100, 40), (130, 33)])
def test_outputs_equal_with_table_without_and_padded(dev, encs, B, L):
    cfg, enc_t, enc_n = encs
    ids, mask = _batch(B, L)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    keep_np = _kept(mask)
    assert keep_np[[3, 7]].all() and keep_np[13].sum() == 1 and keep_np.mean() < 0.9
    keep = torch.from_numpy(keep_np).to(dev)
    h0, p0 = enc_n.forward(it, mt)                            # padded form: every row computed, no table
    ht, pt = enc_t.forward(it, mt)                            # the padded form of the handle with a table never reads it
    assert torch.equal(ht, h0) and torch.equal(pt, p0)
    for name, enc in (("table", enc_t), ("no table", enc_n)):
        hn, p_only = enc.forward(it, mt, ragged=True, want_hidden=False, live_rows_hint=int(keep_np.sum()))
        h_hp, p_hp = enc.forward(it, mt, ragged=True)
        h_only, pn = enc.forward(it, mt, ragged=True, want_pooled=False, live_rows_hint=int(keep_np.sum()))
        assert hn is None and pn is None
        assert torch.equal(p_only, p0), f"{name}: pooled-only"
        assert torch.equal(p_hp, p0), f"{name}: pooled of hidden + pooled"
        assert torch.equal(h_hp[keep], h0[keep]), f"{name}: kept hidden rows"
        assert int((h_hp[~keep] != 0).sum().item()) == 0, f"{name}: dropped rows are zero"
        assert torch.equal(h_only, h_hp), f"{name}: hidden-only"


def _launches(enc, it, mt, **kw):
    from gdr_amd._ffi import lib
    enc.forward(it, mt, ragged=True, **kw)                    # workspace allocated, knobs read
    n0 = lib().gdr_launch_count()
    enc.forward(it, mt, ragged=True, **kw)
    return lib().gdr_launch_count() - n0


@pytest.mark.parametrize("kw", [dict(), dict(want_hidden=False)], ids=["hidden", "pooled_only"])
def test_only_the_unsplit_form_reads_the_table(dev, encs, kw):
    """(64, 40) runs on the split forms: launch for launch as without a table.  (100, 40): block 0's norm and qkv linear are gone and
    the table gather rides in the embedding's launch — two launches fewer."""
    _, enc_t, enc_n = encs
    ids, mask = _batch(64, 40)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    assert _launches(enc_t, it, mt, **kw) == _launches(enc_n, it, mt, **kw)
    ids, mask = _batch(100, 40)
    it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
    assert _launches(enc_t, it, mt, **kw) == _launches(enc_n, it, mt, **kw) - 2


CHILD = r"""
import hashlib, json, sys, torch
sys.path.insert(0, sys.argv[1])
from gdr_amd import ops, synth
from gdr_amd.config import GDRConfig
from gdr_amd._ffi import lib
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
B, L, V = 100, 40, 1000
ids, mask = synth.make_tokens(B, L=L, vocab_hi=V, seed=21, min_len=8)
mask[3] = 0
mask[7, 10:14] = 0
mask[13] = 0
mask[13, 0] = 1
it, mt = torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)
out = {}
for nl in (1, 2):
    cfg = GDRConfig.base(vocab_size=V, num_layers=nl)
    sd = synth.make_state_dict(cfg, seed=31, with_decoder=False)
    for table in (False, True):
        enc = ops.T5EncoderHandle(cfg, sd, dev, token_table=table)
        _, p0 = enc.forward(it, mt)                                       # padded form
        enc.forward(it, mt, want_hidden=False, ragged=True)               # the workspace exists now
        torch.cuda.synchronize()
        for buf in enc.ws.bufs.values():
            buf.fill_(255)                                                # every float of the scratch is a NaN
        n0 = lib().gdr_launch_count()
        _, p = enc.forward(it, mt, want_hidden=False, ragged=True)
        n = lib().gdr_launch_count() - n0
        torch.cuda.synchronize()
        out[f"{nl}/{int(table)}"] = [bool(torch.equal(p, p0)), hashlib.sha256(p.cpu().numpy().tobytes()).hexdigest(), int(n)]
print("RESULT " + json.dumps(out))
"""


def _child(knob):
    env = dict(os.environ, GDR_ENC_LAST_Q_CLS=knob)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_last_block_q_on_cls_rows_is_exact_over_a_nan_workspace():
    """One and two blocks, with and without the table, the workspace all NaN before the call: with one block and no table the q rows
    that are not CLS rows were never written, with two they hold block 0's.  Pooled equals the padded form's in either knob
    setting, the two settings give the same digests, and the knob really switches the launch sequence: norm + k/v linear + gather +
    q linear + scatter instead of norm + qkv linear is three launches more, except where block 0 is the last block and the table
    serves it."""
    off, on = _child("0"), _child("1")
    assert off.keys() == on.keys() and len(off) == 4
    for k in off:
        assert off[k][0] and on[k][0], f"pooled differs from the padded form (num_layers/table = {k})"
        assert off[k][1] == on[k][1], f"GDR_ENC_LAST_Q_CLS changed bits (num_layers/table = {k})"
        assert on[k][2] - off[k][2] == (0 if k == "1/1" else 3), f"launch sequence (num_layers/table = {k})"
