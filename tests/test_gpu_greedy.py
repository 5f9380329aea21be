"""GPU parity of generate() at num_beams = 1 — the reference's default call, its non-beam branch `_generate_no_beam_search`
(generation_utils.py:553-627) — through gdr_t5_generate / gdr_t5_generate_bf16 (csrc/beam.hip greedy_step_kernel): against what the
reference itself returned (g18), against the restatement tests/greedy_ref.py over the CPU oracle, and on crafted weights whose logits
are a small-integer table, where EOS, padding, the early exit and exact ties are all decided by construction.  Ids are compared with
torch.equal unless a test says otherwise."""
import functools
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import greedy_ref
from conftest import golden
from gdr_amd import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release_the_models_at_the_end():
    """The models below live for the module; nothing of them may stay on the device for the modules that follow."""
    yield
    _model.cache_clear()
    _crafted_handle.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _model(kind, bf16=False, table=False, ragged=False, graph=False):
    """One GDRModel per variant for the whole module."""
    from gdr_amd import codec
    from gdr_amd.modeling import GDRModel
    cfg = greedy_ref.CONFIGS[kind]()
    trie = None
    if table:
        V = cfg.output_vocab_size
        if kind == "tiny":   # every third two-digit docid: rows that hit the table and rows that left the trie share a step
            names = ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(0, V * V, 3)]
        else:                # 2 500 clusters of depth 3, as the beam path's table test uses
            names = synth.make_cluster_ids(30000, cluster_size=12, V=V)[0]
        trie = codec.Trie.from_docids(names, V)
    return GDRModel(cfg, greedy_ref.state_dict(kind), torch.device("cuda:0"), prefix_trie=trie, ragged=ragged, graph=graph,
                    dtype=torch.bfloat16 if bf16 else torch.float32)


def _last_done_step():
    from gdr_amd import _ffi
    torch.cuda.synchronize()
    return int(_ffi.lib().gdr_t5_generate_last_done_step())


# ------------------------------------------------------------------------------------------------ 1. the reference's own output
@pytest.mark.parametrize("name", list(greedy_ref.GOLDEN_CASES))
def test_default_generate_call_vs_reference_golden(dev, name):
    g = golden("g18_generate_greedy")
    kind = greedy_ref.GOLDEN_CASES[name][0]
    ids = torch.from_numpy(g[f"{name}_input_ids"].astype(np.int64)).to(dev)
    mask = torch.from_numpy(g[f"{name}_attention_mask"].astype(np.int64)).to(dev)
    ml, ref = int(g[f"{name}_max_length"]), torch.from_numpy(g[f"{name}_ids"])
    model = _model(kind)
    out, none = model.generate(ids, attention_mask=mask, max_length=ml)          # num_beams = num_return_sequences = 1 by default
    assert none is None and torch.is_tensor(out) and out.dtype == torch.int64 and out.shape == ref.shape
    assert torch.equal(out.cpu(), ref)
    out2, enc = model.generate(ids, attention_mask=mask, max_length=ml, output_scores=True, output_encoder_embedding=True)
    assert torch.is_tensor(out2) and torch.equal(out2, out)                      # no scores exist: still the bare tensor
    assert tuple(enc.last_hidden_state.shape) == (ids.shape[0], ids.shape[1], model.config.d_model)   # "expanded" by one
    tabled = _model(kind, table=True)
    out3, _ = tabled.generate(ids, attention_mask=mask, max_length=ml)
    assert torch.equal(out3.cpu(), ref)


# ------------------------------------------------------------------------------------------------ 2. controlled logits
CRAFTED_CALLS = {
    # name: (groups of the rows, width, decode step at which the last row finished — 0: some row never does)
    "eos_at_the_first_step": ([0, 0, 7], 2, 1),
    "eos_at_the_last_step": ([1, 1], 5, 4),
    "never_eos": ([2, 5], 5, 0),
    "all_rows_finished_early": ([0, 3, 4, 3, 7], 3, 2),
    "one_row_finished_among_rows_that_run_on": ([2, 3, 1, 5, 6], 5, 0),
    "eos_ties_with_a_digit": ([4, 7, 4], 3, 2),
    "two_digits_tie": ([5], 5, 0),
    "one_row_early": ([6], 4, 3),
    "one_row_never": ([2], 5, 0),
    "seventy_rows": (list(np.arange(70) % greedy_ref.N_GROUPS), 5, 0),
}


@functools.lru_cache(maxsize=None)
def _crafted_handle():
    from gdr_amd import ops
    cfg, sd, T, Q = greedy_ref.crafted()
    return cfg, sd, T, Q, ops.T5DecoderHandle(cfg, sd, torch.device("cuda:0"))


def _crafted_expectation(groups):
    """The numpy walk over the tables and the restatement over the oracle's step function: they must agree before the GPU is asked."""
    cfg, sd, T, Q, _ = _crafted_handle()
    ml = greedy_ref.CRAFTED_MAX_LENGTH
    ids, lens, ties = greedy_ref.table_walk(T, Q, groups, ml, cfg.output_vocab_size)
    enc, mask = greedy_ref.crafted_encoder_rows(groups, cfg.d_model, cfg.decode_vocab_size)
    o_ids, o_lens = greedy_ref.generate(sd, cfg, None, mask, ml, enc_hidden=enc)
    assert np.array_equal(o_ids.numpy(), ids) and np.array_equal(o_lens.numpy(), lens)
    p_ids, p_lens = greedy_ref.program_rows(groups)
    assert np.array_equal(p_ids, ids) and np.array_equal(p_lens, lens)
    return ids, lens, ties, enc, mask


def _check_crafted_call(dev, name, graph):
    groups, width, done_step = CRAFTED_CALLS[name]
    ml = greedy_ref.CRAFTED_MAX_LENGTH
    ids, lens, ties, enc, mask = _crafted_expectation(groups)
    assert ids.shape[1] == width
    if "tie" in name or name == "seventy_rows":
        assert ties, "the call must decide an exact tie"
    handle = _crafted_handle()[4]
    for _ in range(2 if graph else 1):                                           # captured, then replayed
        out_ids, out_len, out_scores = handle.generate(enc.to(dev), mask.to(dev), 1, ml, 1.0, 1, graph=graph)
    assert tuple(out_ids.shape) == (len(groups), ml) and out_ids.dtype == torch.int64 and out_len.dtype == torch.int32
    want = np.zeros((len(groups), ml), np.int64)
    want[:, :width] = ids                                                        # PAD after EOS, up to max_length
    assert torch.equal(out_ids.cpu(), torch.from_numpy(want))
    assert torch.equal(out_len.cpu().long(), torch.from_numpy(lens))
    assert int(out_len.max()) == width and torch.equal(out_scores.cpu(), torch.zeros(len(groups), dtype=torch.float64))
    if not graph:   # (a replayed graph carries the epoch of its capture: the word is the most recent eager call's business)
        assert _last_done_step() == done_step


@pytest.mark.parametrize("name", list(CRAFTED_CALLS))
def test_controlled_logits_through_the_entry_point(dev, name):
    _check_crafted_call(dev, name, graph=False)


@pytest.mark.parametrize("name", ["all_rows_finished_early", "seventy_rows"])
def test_controlled_logits_through_a_captured_graph(dev, name):
    _check_crafted_call(dev, name, graph=True)


# ------------------------------------------------------------------------------------------------ 3. the early exit changes nothing
CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import greedy_ref
from gdr_amd import _ffi, ops
torch.set_grad_enabled(False)
dev = torch.device("cuda:0")
cfg, sd, T, Q = greedy_ref.crafted()
handle = ops.T5DecoderHandle(cfg, sd, dev)
out = {}
hexed = lambda t: t.cpu().numpy().tobytes().hex()
for name, groups in (("seventy", list(np.arange(70) % greedy_ref.N_GROUPS)), ("mixed", [2, 3, 1, 5, 6]), ("early", [0, 3, 4, 3, 7])):
    enc, mask = greedy_ref.crafted_encoder_rows(groups, cfg.d_model, cfg.decode_vocab_size)
    for rep in range(3):
        ids, lens, scores = handle.generate(enc.to(dev), mask.to(dev), 1, greedy_ref.CRAFTED_MAX_LENGTH, 1.0, 1)
    out[name] = {"ids": hexed(ids), "len": hexed(lens), "scores": hexed(scores)}
torch.cuda.synchronize()
out["early_exits"] = int(_ffi.lib().gdr_t5_generate_early_exits())
out["last_done_step"] = int(_ffi.lib().gdr_t5_generate_last_done_step())     # of the "early" call just above
print("RESULT " + json.dumps(out))
"""


def _run(**env):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def test_leaving_the_step_loop_early_changes_no_byte():
    base, full = _run(), _run(GDR_DECODE_EARLY_EXIT="0")
    base.pop("early_exits")                                   # the host half races with the GPU by design: not asserted
    assert base.pop("last_done_step") == 2                    # every row of the last call had emitted EOS after its second token
    assert full.pop("early_exits") == 0 and full.pop("last_done_step") == 0
    assert full == base, "out_ids, out_len and out_scores must be byte-identical with and without the early exit"


# ------------------------------------------------------------------------------------------------ 4. variants of generate()
def _generate_case(model, name, dev):
    cfg, _, ids, mask, ml, _ = greedy_ref.case_inputs(name)
    out, _ = model.generate(torch.from_numpy(ids).to(dev), attention_mask=torch.from_numpy(mask).to(dev), max_length=ml)
    return out.cpu()


def _assert_fp32_margin(name):
    ref, _, trace = greedy_ref.oracle(name)
    gap = greedy_ref.min_gap(trace)
    print(f"{name}: smallest deciding gap of the restatement {gap:.3e} (need >= {greedy_ref.GAP:g})")
    assert gap >= greedy_ref.GAP
    return ref


def test_long_input_takes_the_key_block_cross_attention(dev):
    ref = _assert_fp32_margin("tiny_200")                                        # L = 200 > 128 keys, B = 2
    assert torch.equal(_generate_case(_model("tiny"), "tiny_200", dev), ref)


def test_graph_replay_equals_the_eager_call(dev):
    ref = _assert_fp32_margin("tiny_graph")
    eager = _generate_case(_model("tiny"), "tiny_graph", dev)
    captured = _generate_case(_model("tiny", graph=True), "tiny_graph", dev)
    replayed = _generate_case(_model("tiny", graph=True), "tiny_graph", dev)
    assert torch.equal(eager, ref) and torch.equal(captured, eager) and torch.equal(replayed, eager)


def test_ragged_encoder_feeds_one_row_per_query(dev):
    ref = _assert_fp32_margin("tiny_ragged")                                     # B = 5 rows of lengths 9, 3, 12, 1, 7
    assert torch.equal(_generate_case(_model("tiny", ragged=True), "tiny_ragged", dev), ref)
    assert torch.equal(_generate_case(_model("tiny"), "tiny_ragged", dev), ref)


# ------------------------------------------------------------------------------------------------ 5. the bf16 precision mode
@pytest.mark.parametrize("name", ["tiny_bf16", "base2_bf16"])
def test_bf16_mode_follows_the_emulation_token_by_token(dev, name):
    """Against the restatement over t5_ref.bf16_linears().  A row may leave the emulation's sequence only at a step whose gap in the
    emulation is below BF16_GAP (5e-3, what hypothesis_lists_match asserts for this mode); a row that has left is not compared further;
    at most a tenth of the rows may leave.  The committed seeds keep the share of rows that have ANY such step below a tenth
    (greedy_ref.BF16_SHARE; tests/test_greedy_host.py)."""
    kind, _, _, ml, _, _ = greedy_ref.ORACLE_CASES[name]
    ref, _, trace = greedy_ref.oracle(name)
    share = float(greedy_ref.close_rows(trace, greedy_ref.BF16_GAP).float().mean())
    assert share < 0.1 and share == pytest.approx(greedy_ref.BF16_SHARE[name], abs=1e-9)
    out = _generate_case(_model(kind, bf16=True), name, dev)
    B = ref.shape[0]
    pad = lambda t: torch.cat([t, torch.zeros((B, ml - t.shape[1]), dtype=torch.int64)], dim=1)   # noqa: E731
    got, want = pad(out), pad(ref)
    left = 0
    for b in range(B):
        diff = torch.nonzero(got[b] != want[b])
        if len(diff):
            s = int(diff[0]) - 1                                                 # the step that decided token s + 1
            gap = float(trace[s][1][b])
            print(f"{name}: row {b} leaves the emulation at step {s} (emulation gap {gap:.3e})")
            assert bool(trace[s][2][b]) and gap < greedy_ref.BF16_GAP, (b, s, gap)
            left += 1
    print(f"{name}: {left} of {B} rows left the emulation's sequence")
    assert left <= 0.1 * B


# ------------------------------------------------------------------------------------------------ 6. sanity against the beam path
@pytest.mark.parametrize("name", list(greedy_ref.GOLDEN_CASES))
def test_first_token_is_the_beam_search_s_best_first_candidate(dev, name):
    g = golden("g18_generate_greedy")
    kind = greedy_ref.GOLDEN_CASES[name][0]
    model = _model(kind)
    ids = torch.from_numpy(g[f"{name}_input_ids"].astype(np.int64)).to(dev)
    mask = torch.from_numpy(g[f"{name}_attention_mask"].astype(np.int64)).to(dev)
    ml = int(g[f"{name}_max_length"])
    out, _ = model.generate(ids, attention_mask=mask, max_length=ml)
    enc_h, _ = model.enc.forward(ids, mask, want_pooled=False)
    _, _, _, _, tt = model.dec.generate(enc_h, mask, 2, ml, 1.0, 2, trace=True)
    assert torch.equal(tt[0, :, 0].long() % model.config.decode_vocab_size, out[:, 1])
