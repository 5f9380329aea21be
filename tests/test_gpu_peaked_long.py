"""The peaked cases of tests/peaked.py that test_gpu_peaked.py does not reach, against the oracle in float64 under that file's rules (fp32
paths: max(1e-4, 4 g) with the recorded g; bf16 mode: 4 x the recorded noise of the emulation; ids by hypothesis_lists_match).

More than 128 keys — the key-block forms of csrc/attention_long.hip, an online softmax over blocks of 64 keys for blocks of 128 queries,
and attention_kernel<8> for other head widths.  Softmax is shift-invariant: with near-uniform probabilities a running maximum taken over
the wrong lanes or not carried from one key block to the next still gives the right quotient.  Here the row maximum lies behind key
block 0 in most rows and carries real weight, and in enc-long-steep it climbs or falls by more than ln(FLT_MAX) between blocks, where a
stale maximum overflows.  No sequence here has an all-zero mask (fp32 quantises -1e9 + s to steps of 64, float64 does not: those rows
stay with the fp32-oracle tests of test_gpu_t5_long.py).

Under 128 keys — the instantiations of the one-pass kernels that no case of test_gpu_peaked.py reaches; each sizes its own LDS image.
Each test names the kernel form its shape reaches through launch_attention (csrc/attention.hip) and prints its measured maximum error."""
import numpy as np
import pytest
import torch

import peaked as P
from peaked_gpu import FP32_SETTINGS, close as _close, generate_vs_oracle as _generate_vs_oracle, pooled_close as _pooled_close
from peaked_gpu import statistics_close as _statistics_close, to_dev as _dev, tower as _tower

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _kept(mask):
    """The rows the ragged entry computes: the live ones, and every row of a sequence whose mask is no prefix of ones."""
    keep = mask != 0
    for b in range(len(mask)):
        if not mask[b, :int(mask[b].sum())].all():
            keep[b] = True
    return keep


def _both_entries_vs(enc, dev, ids, mask, ref, bound, what):
    """Padded entry: every row, PAD rows included, and pooled.  Ragged entry: kept rows and pooled, torch.equal to the padded entry's;
    dropped rows zero."""
    it, mt = _dev(ids, dev), _dev(mask, dev)
    keep = _kept(mask)
    h0, p0 = enc.forward(it, mt)
    h1, p1 = enc.forward(it, mt, ragged=True, live_rows_hint=int(keep.sum()))
    got = h0.cpu().numpy()
    assert np.isfinite(got).all(), what + ": non-finite hidden states"
    _close(got, ref, bound, what + " padded hidden")
    _close(p0.cpu().numpy(), ref[:, 0], bound, what + " padded pooled")
    _close(h1.cpu().numpy()[keep], ref[keep], bound, what + " ragged hidden (kept rows)")
    kd = _dev(keep, dev)
    assert torch.equal(h1[kd], h0[kd]) and torch.equal(p1, p0), what + ": the ragged entry differs from the padded one on kept rows"
    assert int((h1[~kd] != 0).sum()) == 0, what + ": dropped rows must be zero"


# ------------------------------------------------------------------------------------------------------------ T5 encoder, L > 128
@pytest.mark.parametrize("st", FP32_SETTINGS)
@pytest.mark.parametrize("name", list(P.ENCODER_LONG_CASES))
def test_peaked_long_encoder_vs_float64_oracle(dev, name, st):
    """enc-long: d_kv = 64 — attention_long_f32_kernel<LONG_T5_SELF>.  L = 200 (lengths 200, 129, 131, 17: key blocks 64 + 64 + 64 + 8,
    two query blocks) and L = 512 (512, 385, 140, 1, a left-padded row whose first 200 keys are masked and a row with a hole at keys
    130..389); >= 256 token rows, so the ragged entry runs its packed kernels (seq_off / seq_len).
    enc-long-generic: d_kv = 16, L = 300 (300, 129, 17, 1) — attention_kernel<8>; its ragged entry is the padded forward with the
    dropped rows zeroed."""
    from gdr_amd import ops
    cfg, sd, inputs = P.encoder_case(name, st)
    bound = P.fp32_bound(P.ENCODER_LONG_CASES[name]["g"][st.name])
    enc = ops.T5EncoderHandle(cfg, sd, dev)
    ref = P.encoder_oracle(name, st, True)
    for L, (ids, mask) in inputs.items():
        _both_entries_vs(enc, dev, ids, mask, ref[L], bound, f"{name} {st.name} L={L}")


def test_peaked_long_encoder_steep_vs_float64_oracle(dev):
    """enc-long-steep: the L = 512 batch of enc-long at STRONG with the saturated buckets of the position bias raised by 110 (steep_t5)
    — attention_long_f32_kernel<LONG_T5_SELF>, whose block loop LONG_PLAIN and LONG_T5_CROSS share.  On heads 0 and 1 the row maximum
    of an early query arrives in a late key block, more than ln(FLT_MAX) above everything before it: alpha = exp(m - m_new) underflows
    to 0 and wipes the running sum, and exp(score - m) against a maximum that was not raised is inf.  On heads 2 and 3 it arrives in
    an early block and every later block adds exp(-100) = 0.  Both entries."""
    from gdr_amd import ops
    cfg, sd, ids, mask = P.steep_case()
    _both_entries_vs(ops.T5EncoderHandle(cfg, sd, dev), dev, ids, mask, P.steep_oracle(True), P.fp32_bound(P.ENC_LONG_STEEP["g"]),
                     "enc-long-steep")


# ------------------------------------------------------------------------------------------------------------ doc tower, L > 128
@pytest.mark.parametrize("st", FP32_SETTINGS)
def test_peaked_long_doc_tower_vs_float64_oracle(dev, st):
    """bert-long: 2 heads of 64, L = 384 (lengths 384, 129, 200, 17, 1) — attention_long_f32_kernel<LONG_PLAIN> with scale = 1/8.  Padded
    on the 5 passages; ragged on the 5 tiled to 192 GEMM tiles of 128 token rows (the packed kernels' threshold in bert.hip), oracle
    on the 5."""
    name = "bert-long"
    bc, sd, (ids, mask) = P.bert_case(name, st)
    bound = P.fp32_bound(P.BERT_LONG_CASES[name]["g"][st.name])
    ref = P.bert_oracle(name, st, True)
    tower = _tower(bc, sd, dev)
    hid, pooled = tower.bert.forward(_dev(ids, dev), _dev(mask, dev), ragged=False)
    _close(hid.cpu().numpy(), ref, bound, f"{name} {st.name} padded hidden")
    _close(pooled.cpu().numpy(), ref[:, 0], bound, f"{name} {st.name} padded pooled")
    reps = -(-(191 * 128 + 1) // ids.size)
    assert -(-(reps * ids.size) // 128) >= 192
    ti, tm = np.tile(ids, (reps, 1)), np.tile(mask, (reps, 1))
    hid, pooled = tower.bert.forward(_dev(ti, dev), _dev(tm, dev), ragged=True, live_rows_hint=int(tm.sum()))
    got, keep = hid.cpu().numpy(), tm != 0
    _close(got[keep], np.tile(ref, (reps, 1, 1))[keep], bound, f"{name} {st.name} ragged x{reps} hidden (kept rows)")
    _close(pooled.cpu().numpy(), np.tile(ref[:, 0], (reps, 1)), bound, f"{name} {st.name} ragged x{reps} pooled")
    assert not got[~keep].any()


def test_peaked_long_doc_tower_bf16_mode_vs_float64_emulation(dev):
    """bert-long-bf16: the bert-long inputs in the bf16 mode at MODERATE — attention_long_bf16_kernel, a body of its own (bf16 MFMAs,
    probabilities split exactly into three bf16 pieces).  Kept rows; 4 x the noise maximum exceeds the 3e-2 cap as for bert-bf16, so
    the case is held to that case's statistics as well."""
    st = P.bf16_setting(P.BERT_LONG_BF16)
    bc, sd, (ids, mask) = P.bert_case(P.BERT_LONG_BF16["case"], st)
    ref = P.bert_oracle(P.BERT_LONG_BF16["case"], st, True, True)
    hid, pooled = _tower(bc, sd, dev, dtype=torch.bfloat16).bert.forward(_dev(ids, dev), _dev(mask, dev))
    got, keep = hid.cpu().numpy(), mask != 0
    _statistics_close(got[keep], ref[keep], P.BERT_LONG_BF16, "bert-long-bf16 hidden (kept rows)")
    _pooled_close(pooled.cpu().numpy(), ref[:, 0], P.BERT_LONG_BF16, "bert-long-bf16 pooled")
    assert not got[~keep].any()


# ------------------------------------------------------------------------------------------------------------ generate, L > 128
@pytest.mark.parametrize("name,sname", P.case_settings(P.GENERATE_LONG_CASES))
def test_peaked_long_generate_vs_float64_oracle(dev, name, sname):
    """gen-long ((B, R, L) = (3, 6, 300), lengths 300, 129, 200, d_model = 256): attention_long_f32_kernel<LONG_T5_CROSS> with step 0's
    single row and then a 6-row tile whose q rows are slab-sourced — at d_model = 256 the q projection of the 18 beam rows is split
    into 2 K slabs (linear_f32_small_splits: S <= d_model / 128) and decode.hip hands them to the kernel un-reduced (q_part); the
    encoder through <LONG_T5_SELF>.
    gen-long-wide ((12, 130, 129), 12 docid symbols, d_model = 128, MODERATE): finished q rows (d_model = 128 is never split) in two
    query blocks (128 + 2 beam rows) over key blocks of 64 + 64 + 1.  At STRONG no token seed from 1 to 50 keeps the tied share of
    the float64 search under 5 % at 130 beams (peaked.py), so STRONG runs as gen-long-wide-64 at (24, 64, 129): finished q rows,
    one query block — the two-query-block walk is held at MODERATE only."""
    _generate_vs_oracle(dev, name, P.SETTINGS[sname], name)


# ------------------------------------------------------------------------------------------------------------ under 128 keys
@pytest.mark.parametrize("st", FP32_SETTINGS)
def test_peaked_encoder_mfma_tiles_vs_float64_oracle(dev, st):
    """enc-mfma-tiles: d_kv = 64 at L = 16, 64, 65, 96, 112 — attention_mfma16_kernel<1>, <4>, <5>, <6>, <7>.  Sequence lengths 1, 16, 17
    (where <= L) and L; every row of the padded form."""
    from gdr_amd import ops
    name = "enc-mfma-tiles"
    cfg, sd, inputs = P.encoder_case(name, st)
    bound = P.fp32_bound(P.ENCODER_TILE_CASES[name]["g"][st.name])
    enc = ops.T5EncoderHandle(cfg, sd, dev)
    ref = P.encoder_oracle(name, st, True)
    for L, (ids, mask) in inputs.items():
        hid, pooled = enc.forward(_dev(ids, dev), _dev(mask, dev))
        _close(hid.cpu().numpy(), ref[L], bound, f"{name} {st.name} L={L} hidden")
        _close(pooled.cpu().numpy(), ref[L][:, 0], bound, f"{name} {st.name} L={L} pooled")


def test_peaked_encoder_bf16_tiles_vs_float64_emulation(dev):
    """enc-bf16-tiles: the bf16 mode at the enc-bf16 setting (MODERATE with q x 3), padded, at L = 16 and L = 128 —
    attention_mfma_bf16_kernel<1> and <8>.  Held to the noise over both shapes; 4 x its maximum exceeds the 3e-2 cap, so to the
    statistics of bert-bf16 as well."""
    from gdr_amd import ops
    st = P.bf16_setting(P.ENC_BF16_TILES)
    name = P.ENC_BF16_TILES["case"]
    cfg, sd, inputs = P.encoder_case(name, st)
    enc = ops.T5EncoderHandle(cfg, sd, dev, dtype=torch.bfloat16)
    ref = P.encoder_oracle(name, st, True, True)
    got = {}
    for L, (ids, mask) in inputs.items():
        hid, pooled = enc.forward(_dev(ids, dev), _dev(mask, dev))
        got[L] = hid.cpu().numpy()
        print(f"enc-bf16-tiles L={L}: max |gpu - bf16 emulation with float64 sums| {np.abs(got[L] - ref[L]).max():.3e}")
        _pooled_close(pooled.cpu().numpy(), ref[L][:, 0], P.ENC_BF16_TILES, f"enc-bf16-tiles L={L} pooled")
    _statistics_close(np.concatenate([got[L].ravel() for L in got]), np.concatenate([ref[L].ravel() for L in got]), P.ENC_BF16_TILES,
                      "enc-bf16-tiles hidden (both shapes)")


@pytest.mark.parametrize("name,sname", P.case_settings(P.GENERATE_TILE_CASES))
def test_peaked_generate_tiles_vs_float64_oracle(dev, name, sname):
    """gen-cross-16, gen-cross-128: the gen-cross-mfma shape (80 x 20 = 1 600 beam rows) at L = 16 and L = 128 —
    attention_cross_mfma16_kernel<1> and <8>.
    gen-heads4-16: gen-heads4 (128 x 32 = 4 096 rows x 4 heads) with 17 output positions — the steps whose self-attention sees 13 .. 16
    keys: attention_decode_heads4_kernel<16> (the host test holds the search open that long).  At STRONG 13 % of the float64 beam rows
    lie inside a tie group (recorded and re-asserted by the host test): every beam score is held to the bound, the ids by position
    outside those groups."""
    _generate_vs_oracle(dev, name, P.SETTINGS[sname], name)
