"""The peaked-softmax cases of tests/peaked.py on the CPU, on the exact inputs a GPU parity test of these cases takes from there: they ARE peaked (a later change
to synth must not turn them uniform again unnoticed), the recorded distance g between the fp32 and the float64 oracle still holds (the GPU
bounds are 4 g), the bf16 mode's recorded noise still holds, and the float64 beam scores leave at most 5 % of the beam rows inside the tie
window of the id comparison."""
import numpy as np
import pytest
import torch

import peaked as P

torch.set_grad_enabled(False)
SETTING_NAMES = ["moderate", "strong"]


def _assert_peaked(scores, setting, what):
    for top, prob in map(P.score_stats, scores):
        print(f"{what} {setting.name}: max |score| {top:.1f}, mean top probability of block 0 {prob:.2f}")
        assert prob >= P.MIN_TOP_PROB and top >= setting.min_score, (what, setting.name, top, prob)


def _assert_recorded(measured, recorded, what):
    print(f"{what}: measured {measured:.3e}, recorded {recorded:.3e}")
    assert recorded / 1.5 <= measured <= recorded * 1.5, (what, measured, recorded)


@pytest.mark.parametrize("sname", SETTING_NAMES)
@pytest.mark.parametrize("name", list(P.ENCODER_CASES))
def test_encoder_case_is_peaked_and_keeps_its_oracle_gap(name, sname):
    _encoder_premises(name, sname, P.ENCODER_CASES)


def _assert_walks_blocks(scores, mask, what):
    """More than 128 keys: the row maximum of most rows lies behind key block 0, so an online softmax over 64-key blocks has to raise
    its running maximum and rescale what it has summed."""
    after0 = P.block_walk_stats(scores, mask)[2]
    print(f"{what}: the row maximum lies behind key block 0 in {100 * after0.mean():.0f} % of the live rows of the sequences over 128")
    assert after0.mean() >= 0.5, what


def _encoder_premises(name, sname, table):
    st = P.SETTINGS[sname]
    cfg, sd, inputs = P.encoder_case(name, st)
    scores = {L: P.t5_block0_scores(sd, cfg, i, m) for L, (i, m) in inputs.items()}
    _assert_peaked(scores.values(), st, name)
    for L, (_, mask) in inputs.items():
        assert mask.any(1).all(), "a float64 comparison holds no sequence whose mask is all zero"
        if L > 128:
            _assert_walks_blocks(scores[L], mask, f"{name} {sname} L={L}")
    h32, h64 = P.encoder_oracle(name, st, False), P.encoder_oracle(name, st, True)
    _assert_recorded(max(float(np.abs(h32[L] - h64[L]).max()) for L in h32), table[name]["g"][sname], f"{name} {sname} g")


@pytest.mark.parametrize("sname", SETTING_NAMES)
@pytest.mark.parametrize("name", list(P.ENCODER_LONG_CASES) + ["enc-mfma-tiles"])
def test_long_and_tile_encoder_case_is_peaked_and_keeps_its_oracle_gap(name, sname):
    """enc-long (L = 200, 512: attention_long_f32_kernel<LONG_T5_SELF>), enc-long-generic (L = 300, d_kv 16: attention_kernel<8>) and
    enc-mfma-tiles (L = 16 .. 112: attention_mfma16_kernel<1, 4, 5, 6, 7>): the premises of the cases under 128 keys, and above 128
    keys the row maximum behind key block 0 in most rows."""
    _encoder_premises(name, sname, P.ENCODER_LONG_CASES if name in P.ENCODER_LONG_CASES else P.ENCODER_TILE_CASES)


def test_steep_encoder_case_climbs_and_falls_past_the_fp32_exponent_range():
    """enc-long-steep: in float64, over the live rows of the sequences longer than 128, the row maximum exceeds the maximum over keys
    0..63 by >= 100 in at least 10 % of the rows of heads 0 and 1 (climb), and exceeds the maximum over the row's last visited key
    block by >= 100 in at least 10 % of the rows of heads 2 and 3 (fall): exp(score - m) against a running maximum that was not
    carried from block to block, or was taken over the wrong lanes, overflows fp32 (ln FLT_MAX = 88.7).  g as everywhere."""
    t = P.ENC_LONG_STEEP
    cfg, sd, ids, mask = P.steep_case()
    assert mask.any(1).all()
    scores = P.t5_block0_scores(P.as_float64(sd), cfg, ids, mask)
    top, prob = P.score_stats(scores)
    climb, fall, _ = P.block_walk_stats(scores, mask)
    up, down = (climb >= t["step"]).mean(0), (fall >= t["step"]).mean(0)
    print(f"enc-long-steep: max |score| {top:.1f}, mean top probability of block 0 {prob:.2f}; share of rows per head with climb >= "
          f"{t['step']:g}: {np.round(up, 3).tolist()}, with fall >= {t['step']:g}: {np.round(down, 3).tolist()} ({len(climb)} rows)")
    assert prob >= P.MIN_TOP_PROB and top >= t["step"]
    assert (up[:2] >= t["min_share"]).all() and (down[2:4] >= t["min_share"]).all(), (up, down)
    _assert_recorded(float(np.abs(P.steep_oracle(False) - P.steep_oracle(True)).max()), t["g"], "enc-long-steep g")


@pytest.mark.parametrize("sname", SETTING_NAMES)
@pytest.mark.parametrize("name", list(P.BERT_CASES))
def test_doc_tower_case_is_peaked_and_keeps_its_oracle_gap(name, sname):
    _doc_tower_premises(name, sname, P.BERT_CASES)


def _doc_tower_premises(name, sname, table):
    st = P.SETTINGS[sname]
    bc, sd, (ids, mask) = P.bert_case(name, st)
    assert mask.any(1).all(), "a float64 comparison holds no sequence whose mask is all zero"
    scores = P.bert_block0_scores(sd, bc, ids, mask)
    _assert_peaked([scores], st, name)
    if mask.shape[1] > 128:
        _assert_walks_blocks(scores, mask, f"{name} {sname}")
    _assert_recorded(float(np.abs(P.bert_oracle(name, st, False) - P.bert_oracle(name, st, True)).max()),
                     table[name]["g"][sname], f"{name} {sname} g")


@pytest.mark.parametrize("sname", SETTING_NAMES)
@pytest.mark.parametrize("name", list(P.BERT_LONG_CASES))
def test_long_doc_tower_case_is_peaked_and_keeps_its_oracle_gap(name, sname):
    """bert-long (2 heads of 64, L = 384: attention_long_f32_kernel<LONG_PLAIN>)."""
    _doc_tower_premises(name, sname, P.BERT_LONG_CASES)


@pytest.mark.parametrize("sname", SETTING_NAMES)
@pytest.mark.parametrize("name", list(P.GENERATE_CASES))
def test_generate_case_is_peaked_keeps_its_oracle_gap_and_ranks_apart(name, sname):
    """Encoder block 0 at the issue's thresholds; the decode chain at its first step: decoder block 0's cross-attention and the head's
    distribution over the docid columns both with a mean top probability >= 0.5."""
    _generate_premises(name, sname)


def _generate_premises(name, sname):
    st = P.SETTINGS[sname]
    cfg, sd, ids, mask, R = P.generate_case(name, st)
    assert mask.any(1).all(), "a float64 comparison holds no sequence whose mask is all zero"
    _assert_peaked([P.t5_block0_scores(sd, cfg, ids, mask)], st, name + " encoder")
    (cross_top, cross_prob), head_prob = P.decode_step0_stats(sd, cfg, ids, mask)
    print(f"{name} {sname} step 0: cross-attention max |score| {cross_top:.1f}, mean top probability {cross_prob:.2f}; head mean top "
          f"probability {head_prob:.2f}")
    assert cross_prob >= P.MIN_TOP_PROB and head_prob >= P.MIN_TOP_PROB
    s32, (l64, s64) = P.generate_oracle(name, st, False)[1], P.generate_oracle(name, st, True)[:2]
    g = P.generate_row(name)["g"][sname]
    _assert_recorded(float(np.abs(s32 - s64).max()), g, f"{name} {sname} g")
    if name == "gen-rows":       # the search must still be open in the steps that reach attention_decode_rows_kernel (more than 16 keys)
        assert max(len(h) for q in l64 for h in q) >= 18
    if name == "gen-heads4-16":  # ... and in the steps that reach attention_decode_heads4_kernel<16> (13 .. 16 keys)
        assert max(len(h) for q in l64 for h in q) >= 16
    share = P.tied_row_share(s64, P.fp32_bound(g))
    print(f"{name} {sname}: {100 * share:.2f} % of the beam rows within 2 x {P.fp32_bound(g):.1e} of a neighbour; scores "
          f"{s64.min():.2f} .. {s64.max():.2f}")
    tied = P.generate_row(name).get("tied", {}).get(sname)
    if tied is None:
        assert share <= 0.05, share
    else:            # a row that records a larger share (peaked.py says why) keeps it
        _assert_recorded(share, tied, f"{name} {sname} tied share")


@pytest.mark.parametrize("name,sname", P.case_settings(P.GENERATE_LONG_CASES) + P.case_settings(P.GENERATE_TILE_CASES))
def test_long_and_tile_generate_case_is_peaked_keeps_its_oracle_gap_and_ranks_apart(name, sname):
    """gen-long, gen-long-wide and gen-long-wide-64 (more than 128 encoder keys: attention_long_f32_kernel<LONG_T5_CROSS>), gen-cross-16 /
    -128 (attention_cross_mfma16_kernel<1>, <8>) and gen-heads4-16 (attention_decode_heads4_kernel<16>; the search still open at 16
    output positions): the premises of the generate cases above, at the settings each row of peaked.py names."""
    _generate_premises(name, sname)


def _assert_noise(d, table, what):
    print(f"{what} (q x {table['s']:g}): |emulation fp32 sums - emulation float64 sums| max {d.max():.3e} mean {d.mean():.3e}")
    _assert_recorded(float(d.max()), table["noise"][0], what + " max")
    _assert_recorded(float(d.mean()), table["noise"][1], what + " mean")


def test_encoder_bf16_case_noise_and_peakedness():
    """enc-bf16: MODERATE with the q scale lowered to ENC_BF16['s'] (see peaked.py) — still peaked, scores in the tens."""
    st = P.bf16_setting(P.ENC_BF16)
    cfg, sd, inputs = P.encoder_case(P.ENC_BF16["case"], st)
    (top, prob), = [P.score_stats(P.t5_block0_scores(sd, cfg, i, m)) for i, m in inputs.values()]
    print(f"enc-bf16: max |score| {top:.1f}, mean top probability {prob:.2f}")
    assert prob >= P.MIN_TOP_PROB and top >= 15.0
    e32, e64 = P.encoder_oracle(P.ENC_BF16["case"], st, False, True), P.encoder_oracle(P.ENC_BF16["case"], st, True, True)
    _assert_noise(np.concatenate([np.abs(e32[L] - e64[L]).ravel() for L in e32]), P.ENC_BF16, "enc-bf16 noise")
    assert 4 * P.ENC_BF16["noise"][0] <= 3e-2


def test_doc_tower_bf16_case_noise():
    """bert-bf16, kept rows.  4 x max exceeds the 3e-2 cap at every q scale down to 1 (peaked.py states the figures), so next to max and
    mean the case records the 99th percentile, whose 4 x meets the cap, and the share of elements over a quarter of the cap."""
    st = P.bf16_setting(P.BERT_BF16)
    _, _, (_, mask) = P.bert_case(P.BERT_BF16["case"], st)
    d = np.abs(P.bert_oracle(P.BERT_BF16["case"], st, False, True) - P.bert_oracle(P.BERT_BF16["case"], st, True, True))[mask != 0]
    _assert_noise(d, P.BERT_BF16, "bert-bf16 noise")
    _assert_recorded(float(np.quantile(d, 0.99)), P.BERT_BF16["p99"], "bert-bf16 noise 99th percentile")
    _assert_recorded(float((d > 3e-2 / 4).mean()), P.BERT_BF16["over"], "bert-bf16 share of elements with noise > 7.5e-3")
    assert 4 * P.BERT_BF16["p99"] <= 3e-2


def _assert_noise_statistics(d, table, what):
    """The rule of bert-bf16 where 4 x the noise maximum exceeds the 3e-2 cap: the 99th percentile, whose 4 x meets the cap, and the share
    of elements over a quarter of the cap."""
    _assert_noise(d, table, what)
    _assert_recorded(float(np.quantile(d, 0.99)), table["p99"], what + " 99th percentile")
    _assert_recorded(float((d > 3e-2 / 4).mean()), table["over"], what + " share of elements with noise > 7.5e-3")
    assert 4 * table["noise"][0] > 3e-2 >= 4 * table["p99"]


def test_long_doc_tower_bf16_case_noise():
    """bert-long-bf16 (attention_long_bf16_kernel), kept rows: 4 x the noise maximum exceeds the 3e-2 cap as it does for bert-bf16, so
    the case records that case's statistics."""
    st = P.bf16_setting(P.BERT_LONG_BF16)
    _, _, (_, mask) = P.bert_case(P.BERT_LONG_BF16["case"], st)
    d = np.abs(P.bert_oracle(P.BERT_LONG_BF16["case"], st, False, True) - P.bert_oracle(P.BERT_LONG_BF16["case"], st, True, True))
    _assert_noise_statistics(d[mask != 0], P.BERT_LONG_BF16, "bert-long-bf16 noise")


def test_encoder_bf16_tiles_case_noise_and_peakedness():
    """enc-bf16-tiles (attention_mfma_bf16_kernel<1>, <8>): the premise of enc-bf16 at both shapes; the noise maximum (one flipped
    bf16 rounding) x 4 exceeds the 3e-2 cap here, so the case records the statistics of bert-bf16 as well."""
    st = P.bf16_setting(P.ENC_BF16_TILES)
    name = P.ENC_BF16_TILES["case"]
    cfg, sd, inputs = P.encoder_case(name, st)
    for L, (i, m) in inputs.items():
        top, prob = P.score_stats(P.t5_block0_scores(sd, cfg, i, m))
        print(f"enc-bf16-tiles L={L}: max |score| {top:.1f}, mean top probability {prob:.2f}")
        assert prob >= P.MIN_TOP_PROB and top >= 15.0 and m.any(1).all()
    e32, e64 = P.encoder_oracle(name, st, False, True), P.encoder_oracle(name, st, True, True)
    _assert_noise_statistics(np.concatenate([np.abs(e32[L] - e64[L]).ravel() for L in e32]), P.ENC_BF16_TILES, "enc-bf16-tiles noise")


def test_generate_bf16_case_noise():
    """gen-bf16: the noise of a final hypothesis score, on the hypotheses both emulations return."""
    st = P.bf16_setting(P.GEN_BF16)
    l32, s32, _, _ = P.generate_bf16_oracle(st, False)
    l64, s64, _, _ = P.generate_bf16_oracle(st, True)
    gaps = P.shared_score_gaps(l32, s32, l64, s64)
    assert len(gaps) >= 0.9 * s64.size
    _assert_noise(gaps, P.GEN_BF16, "gen-bf16 noise")
    assert 4 * P.GEN_BF16["noise"][0] <= 3e-2


def test_float64_state_dict_keeps_the_bf16_rounding_points():
    """A linear of the emulation under a float64 state dict rounds its operands to bf16 as the fp32 one does; only the sum is wider."""
    from oracle import t5_ref
    cfg, sd, _ = P.encoder_case("enc-mfma", P.MODERATE)
    w = sd["encoder.block.0.layer.0.SelfAttention.k.weight"]
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(1)).standard_normal((3, 5, cfg.d_model)))
    with t5_ref.bf16_linears():
        y = t5_ref._lin(x, w.double())
    assert y.dtype == torch.float64 and torch.equal(y, x.to(torch.bfloat16).double() @ w.to(torch.bfloat16).double().T)
