"""The CPU oracle of the T5 query tower and of generate() above 128 input tokens against the reference's own T5Stack / generate()
(tests/golden/g17_t5_long.npz, made by tests/golden/make_golden_t5_long.py), the bucket table at 512 positions, the input-length
limit of the command line, and the margins of the committed generate() cases: what tests/test_gpu_t5_long.py leans on."""
import numpy as np
import pytest
import torch

import t5_long
from conftest import golden
from oracle import beam_ref, t5_ref

torch.set_grad_enabled(False)


def test_oracle_encoder_matches_reference_at_300_tokens():
    """t64, B = 3, L = 300, lengths 300 / 131 / 17: most offsets lie in the saturated last bucket of either direction."""
    g = golden("g17_t5_long")
    cfg, sd = t5_long.t64(), t5_long.state_dict("t64", int(g["seed"]))
    ids, mask = g["enc_ids"].astype(np.int64), g["enc_mask"].astype(np.int64)
    assert ids.shape == (3, 300) and mask.sum(1).tolist() == [300, 131, 17]
    h = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask)).numpy()
    d = float(np.abs(h[mask != 0] - g["enc_hidden_live"]).max())
    print(f"g17 encoder: oracle vs reference, max |hidden| over live rows {d:.2e}")
    assert d <= 1e-5


def test_oracle_generate_matches_reference_at_200_tokens():
    g = golden("g17_t5_long")
    cfg, sd = t5_long.t64(), t5_long.state_dict("t64", int(g["seed"]))
    ids, mask = torch.from_numpy(g["gen_ids"].astype(np.int64)), torch.from_numpy(g["gen_mask"].astype(np.int64))
    R = int(g["num_beams"])
    assert ids.shape == (2, 200)
    trace = []
    (rd, rs), _ = beam_ref.generate(sd, cfg, ids, mask, R, length_penalty=float(g["length_penalty"]), restricted_head=True, trace=trace)
    assert np.array_equal(rd.numpy(), g["gen_decoded"])
    np.testing.assert_allclose(np.array(rs), g["gen_scores"], rtol=1e-5, atol=1e-5)
    ref_s, ref_t = g["gen_step_scores"], g["gen_step_tokens"]
    assert len(trace) == ref_s.shape[0]
    for s, (sc, tk) in enumerate(trace):
        fin = ref_s[s] > -1e8
        np.testing.assert_allclose(sc.numpy()[fin], ref_s[s][fin], rtol=1e-5, atol=1e-5)
        assert np.array_equal(tk.numpy()[fin], ref_t[s][fin])


@pytest.mark.parametrize("bidirectional,qlen,klen", [(1, 512, 512), (0, 1, 512)])
def test_bucket_table_at_512_positions(bidirectional, qlen, klen):
    from gdr_amd import ops
    got = ops.relative_bucket_table(bidirectional, 32, 128, qlen, klen)
    rel = torch.arange(klen)[None, :] - torch.arange(qlen)[:, None]
    ref = t5_ref.relative_position_bucket(rel, bidirectional=bool(bidirectional), num_buckets=32)
    assert torch.equal(got.to(torch.int64), ref.to(torch.int64))
    if bidirectional:
        assert int((got == 15).sum()) + int((got == 31).sum()) > qlen * klen // 2    # the saturated buckets carry most offsets


@pytest.mark.parametrize("name", sorted(t5_long.GEN_CASES))
def test_committed_generate_cases_clear_the_margin(name):
    """Every cut of the oracle's beam search and every pair of adjacent final scores lies more than 1e-3 apart: ten times the
    tolerance the GPU tests hold scores to, so that equal ids can be asked of them."""
    t5_long.assert_margins(name)


@pytest.mark.parametrize("flag", ["--max_input_length", "--inf_max_input_length"])
def test_cli_refuses_more_than_512_input_tokens(flag):
    from gdr_amd import main, ops
    assert ops.T5_MAX_LEN == 512
    with pytest.raises(SystemExit) as e:
        main.parsers_parser([flag, "513"])
    assert "512" in str(e.value) and flag in str(e.value) and str(e.value).count(".") == 1
    assert getattr(main.parsers_parser([flag, "512", "--mode", "eval"]), flag[2:]) == 512
