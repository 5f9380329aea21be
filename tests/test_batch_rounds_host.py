"""The premises of tests/batch_rounds.py on the CPU: every tower shape runs the packed form and enters the round count it names, the
gather bitmaps hold the designed counts and no sampled query has a reference tie at a cut, the float64 beam search leaves at most
2 % of the beam rows inside the tie window and mixes hit and miss rows inside one thread's rows of prefix_plan_kernel, and every
tolerance of the case table names the test it was taken from or the figure it was measured from."""
import os
import re

import numpy as np
import pytest
import torch

import batch_rounds as BR
import peaked

torch.set_grad_enabled(False)
TESTS = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------------------ pack plan
def test_every_tower_shape_runs_the_packed_form():
    cfg, bc = BR.t5_config(), BR.bert_cfg()
    assert (cfg.d_model, cfg.d_kv, cfg.num_heads, cfg.d_ff, cfg.num_layers) == (128, 64, 4, 256, 2)
    assert (bc["hidden_size"], bc["num_heads"], bc["d_ff"], bc["num_layers"]) == (128, 2, 256, 2)
    for B, L in BR.tower_shapes():
        assert BR.gemm_tiles(B, L, 128) == -(-(B * L) // 128) >= 192, (B, L)       # at these widths the rule is ceil(B L / 128) >= 192
        assert BR.t5_packs(cfg, B, L) and BR.bert_packs(bc, B, L), (B, L)
        assert L <= bc["max_pos"]
    assert not BR.t5_packs(cfg, 1018, BR.TOWER_L) and not BR.bert_packs(bc, 1018, BR.TOWER_L)   # 191 tiles: the rule has teeth here


def test_round_counts_and_chain_split():
    cfg = BR.t5_config()
    assert [BR.rounds(B) for B in BR.TOWER_BATCHES] == [1, 1, 2, 3] and BR.rounds(BR.TOWER_LONG[0]) == 2
    assert 1023 % BR.ROUND and not 1024 % BR.ROUND
    L = BR.TOWER_L
    assert BR.t5_chains(cfg, 1023, L) == (1023,) and BR.t5_chains(cfg, 1024, L) == (1024,)
    assert BR.t5_chains(cfg, 1025, L) == (1025,), "the halves of 1025 do not pack: a pooled-only call stays on one chain of two rounds"
    assert BR.t5_chains(cfg, 2049, L) == (1024, 1025), "pooled-only fp32 at 2049: two chains, each with a plan of its own"
    assert BR.t5_chains(cfg, *BR.TOWER_LONG) == (512, 513)                         # its hidden-output calls stay one chain of two rounds


@pytest.mark.parametrize("B,L", BR.tower_shapes())
def test_masks_around_every_round_boundary(B, L):
    ids, mask = BR.tower_tokens(B, L, 96)
    keep = BR.kept(mask)
    assert ids.shape == mask.shape == (B, L) and ids.min() >= 0 and ids.max() < 96
    for b, pattern in BR.BOUNDARY_PATTERNS.items():
        if b >= B - 1:
            continue
        n = int(mask[b].sum())
        if pattern == "one":
            assert n == 1 and mask[b, 0] == 1 and keep[b].sum() == 1
        elif pattern == "full":
            assert n == L and keep[b].all()
        elif pattern == "zero":
            assert n == 0 and keep[b].all()
        else:
            assert 0 < n < L and mask[b, 0] == 1 and mask[b, -1] == 1 and keep[b].all()
    assert mask[B - 1].tolist() == [1, 1] + [0] * (L - 2) and keep[B - 1].sum() == 2
    lens = keep.sum(1)
    assert lens.min() == 1 and lens.max() == L and keep.mean() < 0.9               # the batch really is ragged
    off = np.concatenate([[0], np.cumsum(lens)])                                   # what pack_scan_kernel must produce
    assert off[-1] == keep.sum() and (B <= BR.ROUND or off[BR.ROUND] > 0)
    assert set(BR.sample_sequences(B)) >= {b for b in (0, 1022, 1023, 1024, 1025, 2047, 2048, B - 1) if b < B}


def test_kept_rows_rule():
    m = np.array([[1, 1, 0, 0], [0, 0, 0, 0], [1, 0, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1], [1, 0, 0, 0]])
    assert BR.kept(m).tolist() == [[1, 1, 0, 0], [1] * 4, [1] * 4, [1] * 4, [1] * 4, [1, 0, 0, 0]]


def test_all_zero_mask_rows_take_the_fp32_mask_semantics():
    """-1e9 absorbs the scores in fp32 only: the float64 oracle of an all-zero mask attends as if the mask were all ones, the fp32
    oracle uniformly.  The sample's oracle therefore holds the fp32 oracle's rows there, and the float64 oracle's everywhere else."""
    from oracle import t5_ref
    B, L = 2049, BR.TOWER_L
    rows, si, sm, keep, ref = BR.tower_sample("t5", B, L)
    j = rows.index(1024)
    assert sm[j].sum() == 0
    cfg, sd = BR.t5_config(), BR.t5_state_dict()
    ti, zeros, ones = torch.from_numpy(np.array(si[j:j + 1])), torch.zeros((1, L), dtype=torch.int64), torch.ones((1, L), dtype=torch.int64)
    f32 = t5_ref.encoder_forward(sd, cfg, ti, zeros).double().numpy()[0]
    f64 = t5_ref.encoder_forward(peaked.as_float64(sd), cfg, ti, zeros).numpy()[0]
    f64_ones = t5_ref.encoder_forward(peaked.as_float64(sd), cfg, ti, ones).numpy()[0]
    assert np.array_equal(ref[j], f32)
    assert np.abs(f64 - f64_ones).max() < 1e-5 < 1e-2 < np.abs(f64 - f32).max()
    others = [i for i in range(len(rows)) if i != j]
    f64_all = t5_ref.encoder_forward(peaked.as_float64(sd), cfg, torch.from_numpy(np.array(si)), torch.from_numpy(np.array(sm))).numpy()
    assert np.array_equal(ref[others], f64_all[others])


# ------------------------------------------------------------------------------------------------------------ tolerances
def _test_exists(test_id):
    path, name = test_id.split("::")
    with open(os.path.join(os.path.dirname(TESTS), path)) as f:
        return re.search(rf"^def {re.escape(name)}\(", f.read(), re.M) is not None


def test_every_tolerance_names_its_source_or_its_measurement():
    for form, row in BR.TOWER_FORMS.items():
        if "source" in row:
            assert _test_exists(row["source"]), (form, row["source"])
            assert row["exact"] or 0 < row["bound"] <= 2e-4
        else:
            assert not row["exact"] and row["margin"] == 4.0 and len(row["measured"]) == 2 and "bound" not in row, form
        if "vs_fp32" in row:
            assert _test_exists(row["vs_fp32_source"]) and 0 < row["vs_fp32"] <= 2e-4, form
    assert _test_exists("tests/test_gpu_query_gather.py::test_four_queries_with_a_filter_each") and BR.GATHER_TOL == 1e-4
    assert _test_exists("tests/test_gpu_prefix.py::test_generate_tiny_with_prefix_table_vs_oracle") and BR.PREFIX_TOL == peaked.fp32_bound(0.0)


def test_doc_tower_bf16_noise_is_the_recorded_one():
    """The measured tolerance of the table: the largest noise over the four L = 24 shapes is the recorded one; no shape exceeds it."""
    noise = [BR.bf16_noise("bert", B, BR.TOWER_L) for B in BR.TOWER_BATCHES]
    for B, (mx, mean) in zip(BR.TOWER_BATCHES, noise):
        print(f"bert-bf16 B={B}: |emulation fp32 sums - emulation float64 sums| max {mx:.3e} mean {mean:.3e}")
    for got, rec in zip((max(n[0] for n in noise), max(n[1] for n in noise)), BR.BERT_BF16_NOISE):
        assert rec / 1.5 <= got <= rec * 1.5, (got, rec)
    assert 4 * BR.BERT_BF16_NOISE[0] <= 3e-2                                       # under the cap tests/peaked.py holds bf16 cases to


# ------------------------------------------------------------------------------------------------------------ gather top-k
@pytest.mark.parametrize("B", BR.GATHER_BATCHES)
def test_gather_bitmaps_hold_the_designed_counts(B):
    a = BR.gather_allowed(B)
    counts = a.sum(1)
    want = BR.gather_designed_counts(B)
    assert {q: int(counts[q]) for q in want} == want and want[B - 1] == 33
    assert all(q in BR.gather_samples(B) for q in want) and 0 in BR.gather_samples(B)
    if B > 1024 and B - 1 != 1024:
        assert a[1024].nonzero()[0].tolist() == [BR.GATHER_N - 1]
    rest = np.delete(counts, list(want))
    assert 0 < rest.min() and rest.max() <= 0.07 * BR.GATHER_N < BR.GATHER_CAP      # 0.2 % .. 5 % of 5000 rows, far under the capacity
    assert (counts > BR.GATHER_CAP).nonzero()[0].tolist() == ([2047] if B > 2047 else [])
    units = -(-np.minimum(counts, BR.GATHER_CAP) // BR.ROWS_UNIT)
    if B > 1025:
        assert units[1025] == 2 and units[2047] == BR.GATHER_CAP // BR.ROWS_UNIT
    assert units[B - 1] == 3
    if B > BR.ROUND:                                                               # the carry into the second round is not zero
        assert units[:BR.ROUND].sum() > 0 and BR.rounds(B) >= 2
    assert BR.GATHER_SLICE <= BR.ROUND and -(-BR.GATHER_CAP // 4096) == 1           # a slice is one round; one chunk of capacity


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", BR.GATHER_BATCHES)
def test_no_sampled_query_has_a_reference_tie_at_a_cut(B, bf16):
    s = BR.gather_case(B, bf16)
    assert s.sample == BR.gather_samples(B) and s.S.shape == (len(s.sample), BR.GATHER_N)
    assert BR.gather_cut_ties(s, BR.GATHER_CAP) == [], "the gather list (first 4096 allowed rows)"
    assert BR.gather_cut_ties(s, 2 ** 20) == [], "the dense list (every allowed row)"
    seed = BR.GATHER_QSEED[(B, bf16)]
    first = next(sd for sd, bad in BR.scan_gather_seeds(B, bf16, range(1, seed + 1)) if not bad)
    assert first == seed, "the table says: the first seed from 1 on without such a tie"


# ------------------------------------------------------------------------------------------------------------ prefix table
@pytest.mark.parametrize("B", list(BR.PREFIX_BATCHES))
def test_prefix_batches_and_the_oracles_own_near_ties(B):
    rows, per, owners = BR.PREFIX_BATCHES[B]
    assert rows == B * BR.PREFIX_R > BR.ROUND and per == -(-rows // BR.ROUND) and owners == -(-rows // per) < BR.ROUND
    assert rows % per == 0 or owners * per > rows
    cfg = BR.prefix_config()
    assert cfg.output_vocab_size == 6 and BR.PREFIX_R <= cfg.output_vocab_size
    lists, sc, trace, ptrace = BR.prefix_oracle(B)
    assert sc.shape == (B, BR.PREFIX_R) and np.isfinite(sc).all() and len(trace) == len(ptrace) == cfg.max_output_length - 1
    share = peaked.tied_row_share(sc, BR.PREFIX_TOL)
    print(f"prefix B={B}: {100 * share:.2f} % of the beam rows lie within the tie window of a neighbour")
    assert share <= BR.PREFIX_MAX_EXCUSED


@pytest.mark.parametrize("keep_every", BR.PREFIX_KEEP_EVERY)
@pytest.mark.parametrize("B", list(BR.PREFIX_BATCHES))
def test_hit_and_miss_rows_share_one_threads_rows(B, keep_every):
    """Levels 0 and 1 of the trie are complete, so the first two steps hit everywhere; at step 2 the holes of the trie split the rows."""
    trie = BR.prefix_trie(keep_every)
    V = trie.V
    assert (trie.child[0] >= 0).all(), "every first digit is a node: complete_levels == 2"
    second = trie.child[trie.child[0]]
    assert (second >= 0).any() and (second < 0).any(), "the second digit level has holes"
    ptrace = BR.prefix_oracle(B)[3]
    assert BR.prefix_hits(trie, ptrace[0]).all() and BR.prefix_hits(trie, ptrace[1]).all()
    steps = BR.prefix_mixed_threads(B, keep_every)
    print(f"prefix B={B} keep_every={keep_every}: (step, mixed threads, hit rows, miss rows) {steps}")
    assert any(mixed > 0 and hits > 0 and misses > 0 for _, mixed, hits, misses in steps)
    assert V == 6


# ------------------------------------------------------------------------------------------------------------ cluster insert
def test_insert_case_spans_three_clusters_per_thread():
    import expand_ref
    offsets, members, new_ids, targets = BR.insert_case()
    C = BR.INSERT_C
    assert C > BR.ROUND and C % BR.ROUND and -(-C // BR.ROUND) == 3 and -(-C // 3) < BR.ROUND
    sizes = np.diff(offsets)
    assert offsets.size == C + 1 and (sizes == 0).sum() > 100 and sizes[[0, 1023, 2047]].tolist() == [0, 0, 0]
    assert new_ids.size == BR.INSERT_NEW == targets.size and (np.diff(new_ids) > 0).all() and new_ids[0] == members.size
    assert targets.min() >= 0 and targets.max() < C and {1023, 1024, 2047, 2048} <= set(targets.tolist())
    o, m = expand_ref.merge(offsets, members, new_ids, targets)
    assert o[-1] == members.size + BR.INSERT_NEW == m.size


def test_remove_case_empties_clusters_and_names_an_absent_id():
    import lifecycle_ref
    offsets, members, ids = BR.remove_case()
    C = BR.INSERT_C
    assert offsets.size == C + 1 and -(-C // BR.ROUND) == 3
    assert (np.diff(ids) > 0).all() and ids[-1] == members.size + 7 and not np.isin(ids[-1], members)
    sizes = np.diff(offsets)
    assert all(sizes[c] > 0 for c in BR.REMOVE_EMPTIED)
    o, m, gone = lifecycle_ref.remove(offsets, members, ids)
    left = np.diff(o)
    assert all(left[c] == 0 for c in BR.REMOVE_EMPTIED) and gone == ids.size - 1 >= 400
    assert o[-1] == m.size == members.size - gone and 0 < left.max() <= sizes.max()
    assert (left < sizes).sum() > 300 and (left == sizes).sum() > 300      # clusters that lose members beside clusters that keep all


# ------------------------------------------------------------------------------------------------------------ k-means partition
def test_partition_cases_sit_on_either_side_of_one_entry_per_thread():
    m = [BR.partition_scan_entries(k, sizes) for k, sizes in BR.PARTITION_CASES]
    assert m == [1024, 1025, 1023] and [-(-x // BR.ROUND) for x in m] == [1, 2, 1]
    assert [(k, len(sizes), sum(sizes)) for k, sizes in BR.PARTITION_CASES] == [(64, 1, 4096), (41, 1, 6400), (33, 31, 7936)]
    assert all(k <= 64 for k, _ in BR.PARTITION_CASES)                     # csrc/kmeans.hip KM_MAX_K
