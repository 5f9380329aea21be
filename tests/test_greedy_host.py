"""The host side of generate() at num_beams = 1 (greedy decode, csrc/beam.hip greedy_step_kernel): the restatement of the reference's
non-beam loop (tests/greedy_ref.py) against what the reference itself returned (g18), the statements the GPU tests rely on about their
CPU-chosen seeds and crafted tables, and the argument checks of the C entry points and the Python surface, which come before any launch
and before any pointer is dereferenced — no GPU needed."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import greedy_ref
from conftest import golden

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ the restatement and its cases
@pytest.mark.parametrize("name", list(greedy_ref.GOLDEN_CASES))
def test_restatement_gives_what_the_reference_returned(name):
    g = golden("g18_generate_greedy")
    cfg, sd, ids, mask, ml = greedy_ref.golden_inputs(name, int(g[f"{name}_token_seed"]))
    assert np.array_equal(ids, g[f"{name}_input_ids"]) and np.array_equal(mask, g[f"{name}_attention_mask"]) and ml == int(g[f"{name}_max_length"])
    assert int(g[f"{name}_token_seed"]) == greedy_ref.GOLDEN_CASES[name][5] and int(g["seed"]) == greedy_ref.SD_SEED
    assert float(g[f"{name}_min_gap"]) >= greedy_ref.GAP          # what the maker asserted of the reference's own logits
    trace = []
    out, lens = greedy_ref.generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), ml, trace=trace)
    ref = g[f"{name}_ids"]
    assert out.dtype == torch.int64 and tuple(out.shape) == ref.shape and np.array_equal(out.numpy(), ref)
    assert int(lens.max()) == ref.shape[1]
    chosen = np.stack([c.numpy() for c, _, _ in trace])
    np.testing.assert_allclose(chosen, g[f"{name}_chosen"], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", list(greedy_ref.ORACLE_CASES))
def test_committed_seeds_keep_their_margins(name):
    """fp32 cases: every deciding step of the restatement clears GAP.  bf16 cases: fewer than a tenth of the rows have a deciding step
    whose gap in the emulation is below BF16_GAP, and the share is the one stored beside the case."""
    _, _, trace = greedy_ref.oracle(name)
    if greedy_ref.ORACLE_CASES[name][5]:
        share = float(greedy_ref.close_rows(trace, greedy_ref.BF16_GAP).float().mean())
        print(f"{name}: share of rows with a deciding gap below {greedy_ref.BF16_GAP:g}: {share:.4f}")
        assert share < 0.1 and share == pytest.approx(greedy_ref.BF16_SHARE[name], abs=1e-9)
    else:
        gap = greedy_ref.min_gap(trace)
        print(f"{name}: smallest deciding gap {gap:.3e}")
        assert gap >= greedy_ref.GAP


def test_crafted_tables_walk_the_program_and_the_oracle_agrees():
    cfg, sd, T, Q = greedy_ref.crafted()
    groups = np.arange(70) % greedy_ref.N_GROUPS
    ml = greedy_ref.CRAFTED_MAX_LENGTH
    ids, lens, ties = greedy_ref.table_walk(T, Q, groups, ml, cfg.output_vocab_size)
    want_ids, want_lens = greedy_ref.program_rows(groups)
    assert np.array_equal(ids, want_ids) and np.array_equal(lens, want_lens)
    # every programmed tie happens, and is decided for the lower token id: EOS against a digit, a digit against a digit
    seen = {(int(groups[b]), p, win, tuple(cols)) for b, p, win, cols in ties}
    assert seen == {(4, 1, 1, (1, 10)), (5, 0, 4, (4, 7)), (7, 0, 1, (1, 3))}
    enc, mask = greedy_ref.crafted_encoder_rows(groups[:greedy_ref.N_GROUPS], cfg.d_model, cfg.decode_vocab_size)
    trace = []
    out, sl = greedy_ref.generate(sd, cfg, None, mask, ml, trace=trace, enc_hidden=enc)
    assert np.array_equal(out.numpy(), want_ids[:greedy_ref.N_GROUPS]) and np.array_equal(sl.numpy(), want_lens[:greedy_ref.N_GROUPS])
    for (b, p, _, _) in [t for t in ties if t[0] < greedy_ref.N_GROUPS]:
        assert float(trace[p][1][b]) == 0.0                     # exact ties in the oracle's own arithmetic as well


def test_greedy_search_pads_finished_rows_and_stops_when_all_are_done():
    Vd = 8
    plan = {0: [3, 1], 1: [4, 5, 1], 2: [1]}                    # per row: the tokens to emit

    def step(seq):
        lg = torch.zeros((3, Vd))
        for b, toks in plan.items():
            k = seq.shape[1] - 1
            lg[b, toks[k] if k < len(toks) else 6] = 1.0         # a finished row's argmax (6) must not show
        return lg
    out, lens = greedy_ref.greedy_search(step, 3, 6)
    assert out.tolist() == [[0, 3, 1, 0], [0, 4, 5, 1], [0, 1, 0, 0]] and lens.tolist() == [3, 4, 2]
    out, lens = greedy_ref.greedy_search(lambda seq: torch.tensor([[0., 0., 5., 5.]]), 1, 4)   # never EOS; ties take the lowest id
    assert out.tolist() == [[0, 2, 2, 2]] and lens.tolist() == [4]


# ------------------------------------------------------------------------------------------------ the C entry points
def _weights(V=30, max_out_len=10):
    from gdr_amd import _ffi
    fake = 0x7f0000000000                      # a non-null "device" pointer: the host code must never dereference it
    dl = (_ffi.GdrT5DecLayer * 2)()
    for ly in dl:
        for f, _t in ly._fields_:
            setattr(ly, f, fake)
    alr = (_ffi.GdrAdaptorLayer * 1)()
    for f, _t in alr[0]._fields_:
        setattr(alr[0], f, fake)
    dims = _ffi.GdrT5Dims(V * max_out_len + 2, 768, 64, 3072, 12, 2, 32, 128, 1e-6)
    w = _ffi.GdrT5DecoderWeights(dims, V, max_out_len, 1, 8, 2048, 1e-5, fake, fake, fake, fake, dl, alr, fake, fake)
    w._keep = (dl, alr)
    return w


def _call(fn, w, B=2, L=16, R=1, ml=10, nret=1, nbytes=1 << 44, trie=False, scores=False, tokens=False, lp=0.8):
    from gdr_amd import _ffi
    p = C.c_void_p(256)                                            # never dereferenced: every call here is refused first
    return fn(C.byref(w), p, p, B, L, R, ml, lp, nret, C.cast(p, C.POINTER(_ffi.GdrTrie)) if trie else None, None, p, p, p,
              p if scores else None, p if tokens else None, C.c_void_p(4096), nbytes, None)


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_one_beam_is_accepted_and_its_contract_is_checked_before_any_launch(which):
    from gdr_amd import _ffi
    l = _ffi.lib()
    fn = (l.gdr_t5_generate, l.gdr_t5_generate_bf16)[which]
    w = _weights()
    for nret in (2, 0, 10):
        assert _call(fn, w, nret=nret) == _ffi.GDR_EINVAL
        msg = l.gdr_last_error()
        assert b"num_return_sequences=%d" % nret in msg and b"num_beams=1" in msg, msg
    for kw, name in ((dict(trie=True), b"trie"), (dict(scores=True), b"step_scores"), (dict(tokens=True), b"step_tokens"),
                     (dict(scores=True, tokens=True), b"step_scores")):
        assert _call(fn, w, **kw) == _ffi.GDR_EINVAL, kw
        msg = l.gdr_last_error()
        assert name in msg and b"NULL" in msg and b"num_beams=1" in msg, msg
    assert _call(fn, w, ml=11) == _ffi.GDR_EINVAL and b"max_length=11" in l.gdr_last_error()
    assert _call(fn, w, ml=1) == _ffi.GDR_EINVAL and b"max_length=1" in l.gdr_last_error()
    assert _call(fn, w, L=513) == _ffi.GDR_EINVAL and b"L=513" in l.gdr_last_error()
    assert _call(fn, w, B=0) == _ffi.GDR_EINVAL
    # an accepted call gets as far as the workspace check, whatever length_penalty says (accepted and unused): one byte short is ENOSPC
    # naming what the size function answers
    for B, L, ml, lp in ((2, 16, 10, 0.8), (1, 1, 2, 1.0), (70, 200, 5, 0.0), (512, 40, 10, -1.0)):
        need = l.gdr_t5_generate_workspace_bytes(C.byref(w), B, L, 1, ml)
        assert need > 0
        assert _call(fn, w, B=B, L=L, ml=ml, nbytes=need - 1, lp=lp) == _ffi.GDR_ENOSPC, (B, L, ml)
        assert int(l.gdr_last_error().decode().rsplit("required", 1)[1]) == need


def test_one_beam_needs_no_more_workspace_than_two():
    from gdr_amd import _ffi
    l = _ffi.lib()
    for V, mol, B, L, ml in ((30, 10, 1, 40, 10), (30, 10, 64, 40, 10), (30, 10, 512, 512, 10), (6, 5, 3, 8, 5), (127, 4, 70, 200, 2)):
        w = _weights(V=V, max_out_len=mol)
        one, two = (l.gdr_t5_generate_workspace_bytes(C.byref(w), B, L, R, ml) for R in (1, 2))
        assert 0 < one <= two, (V, B, L, ml, one, two)


def test_the_table_driven_search_keeps_refusing_one_beam():
    from gdr_amd import _ffi
    l = _ffi.lib()
    p = C.c_void_p(256)
    assert l.gdr_beam_search_table(p, 1, 30, 1, 5, 0.8, 1, None, p, p, p, C.c_void_p(4096), 1 << 44, None) == _ffi.GDR_EINVAL
    assert b"num_beams=1" in l.gdr_last_error()
    w = _weights()
    assert _call(l.gdr_t5_generate, w, R=0, nret=1) == _ffi.GDR_EINVAL and b"num_beams=0" in l.gdr_last_error()


# ------------------------------------------------------------------------------------------------ the Python surface
def _bare_model():
    from gdr_amd.config import GDRConfig
    from gdr_amd.modeling import GDRModel
    m = object.__new__(GDRModel)                                   # no device: the asserts come before anything touches one
    m.config, m.dec = GDRConfig.tiny(), object()
    return m


def test_generate_asserts_one_returned_sequence_with_the_reference_s_message():
    m = _bare_model()
    ids = torch.zeros((2, 4), dtype=torch.long)
    with pytest.raises(AssertionError) as e:
        m.generate(ids, num_return_sequences=2)                   # num_beams defaults to 1, as in the reference
    assert str(e.value) == ("Greedy decoding will always produce the same output for num_beams == 1 and num_return_sequences > 1. "
                            "Please set num_return_sequences = 1")
    with pytest.raises(AssertionError) as e:
        m.generate(ids, num_beams=1, num_return_sequences=3, max_length=5)
    assert "num_return_sequences = 1" in str(e.value)
    with pytest.raises(NotImplementedError):
        m.generate(ids, do_sample=True)


def test_the_retriever_refuses_one_returned_sequence():
    from gdr_amd import _ffi
    from gdr_amd.modeling import GDRRetriever
    args = types.SimpleNamespace(num_return_sequences=1, max_output_length=5, length_penalty=0.8)
    with pytest.raises(_ffi.GdrError) as e:
        GDRRetriever(None, None, None, args)
    msg = str(e.value)
    assert "num_return_sequences" in msg and "greedy" in msg and msg.count(". ") == 0, msg
    args.num_return_sequences = 2
    r = GDRRetriever(None, None, None, args)
    args.num_return_sequences = 1                                  # changed behind the retriever's back: the step refuses as well
    with pytest.raises(_ffi.GdrError):
        r.validation_step_i({"source_ids": torch.zeros((1, 4), dtype=torch.long), "source_mask": None})
