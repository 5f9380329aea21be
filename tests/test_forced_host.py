"""Host side of the teacher-forced decode and the decoder-side stage-2 queries — no GPU: the score mode of gdr_t5_generate /
gdr_t5_generate_bf16 (out_len = NULL) is accepted, checks its contract before any launch and is served by the search's workspace
size; the search's own answers (out_len != NULL) are what they were; GDR_RERANK_ROW_QUERIES is a known flag and its neighbours stay
unknown; the three unimplemented --use_query_embed_* combinations stop before anything runs; and tests/forced_ref.py, the restatement
the GPU tests hold the kernels to, is checked on hand-written cases."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import forced_ref


# ------------------------------------------------------------------------------------------------ the C entry points
def _weights(V=30, max_out_len=10, plain=False):
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
    if plain:
        w = _ffi.GdrT5DecoderWeights(dims, V, max_out_len, 0, 0, 0, 0.0, fake, fake, fake, fake, dl, None, None, fake)
    else:
        w = _ffi.GdrT5DecoderWeights(dims, V, max_out_len, 1, 8, 2048, 1e-5, fake, fake, fake, fake, dl, alr, fake, fake)
    w._keep = (dl, alr)
    return w


def _call(fn, w, B=2, L=16, R=4, ml=10, nret=None, nbytes=1 << 44, trie=False, table=False, lens=False, scores=False, tokens=False,
          lp=0.8):
    """lens=False: out_len = NULL, the score mode."""
    from gdr_amd import _ffi
    p = C.c_void_p(256)                                            # never dereferenced: every call here is refused first
    return fn(C.byref(w), p, p, B, L, R, ml, lp, R if nret is None else nret,
              C.cast(p, C.POINTER(_ffi.GdrTrie)) if trie else None, C.cast(p, C.POINTER(_ffi.GdrPrefixTable)) if table else None,
              p, p if lens else None, p, p if scores else None, p if tokens else None, C.c_void_p(4096), nbytes, None)


def _fns():
    from gdr_amd import _ffi
    l = _ffi.lib()
    return l, (l.gdr_t5_generate, l.gdr_t5_generate_bf16)


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("plain", [False, True], ids=["adaptor", "plain"])
def test_score_mode_is_accepted_and_the_search_s_workspace_size_serves_it(which, plain):
    from gdr_amd import _ffi
    l, fns = _fns()
    w = _weights(plain=plain)
    for R in (1, 4, 1024):          # 1024 rows x 31 columns and a 1024-entry heap: no select and no heap, so neither limit applies
        for hidden in (False, True):
            need = l.gdr_t5_generate_workspace_bytes(C.byref(w), 2, 16, R, 10)
            assert need > 0
            assert _call(fns[which], w, R=R, scores=hidden, nbytes=need - 1) == _ffi.GDR_ENOSPC, (R, hidden, l.gdr_last_error())
            assert int(l.gdr_last_error().decode().rsplit("required", 1)[1]) == need
            # with enough bytes the next check is the alignment of the (fake) workspace pointer 4096: passed, so nothing is left but
            # the launches — not made here
    assert l.gdr_abi_version() == _ffi.ABI_VERSION == 9


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_score_mode_names_the_argument_it_refuses_before_any_launch(which):
    from gdr_amd import _ffi
    l, fns = _fns()
    fn, w = fns[which], _weights()
    for kw, names in ((dict(nret=3), (b"num_return_sequences=3", b"num_beams=4")), (dict(nret=1), (b"num_return_sequences=1",)),
                      (dict(R=1, nret=2), (b"num_return_sequences=2",)),
                      (dict(trie=True), (b"trie", b"NULL")), (dict(table=True), (b"prefix_table", b"NULL")),
                      (dict(tokens=True), (b"step_tokens", b"NULL")), (dict(scores=True, tokens=True), (b"step_tokens",)),
                      (dict(lp=0.0), (b"length_penalty",)), (dict(lp=-1.0), (b"length_penalty",)),
                      (dict(R=0), (b"num_beams=0",)), (dict(R=1025), (b"num_beams=1025", b"1024")),
                      (dict(ml=11), (b"max_length=11",)), (dict(ml=1), (b"max_length=1",)), (dict(L=513), (b"L=513",)),
                      (dict(L=0), (b"L=0",)), (dict(B=0), (b"B=0",))):
        assert _call(fn, w, **kw) == _ffi.GDR_EINVAL, kw
        msg = l.gdr_last_error()
        assert all(n in msg for n in names), (kw, msg)
    # prefix_table with plain-head weights: refused in this mode as well
    assert _call(fn, _weights(plain=True), table=True) == _ffi.GDR_EINVAL and b"prefix_table" in l.gdr_last_error()
    # the mode is selected by out_len alone: the other pointers stay required
    p = C.c_void_p(256)
    assert fn(C.byref(w), p, p, 2, 16, 4, 10, 0.8, 4, None, None, None, None, p, None, None, C.c_void_p(4096), 1 << 44, None) == _ffi.GDR_EINVAL
    assert b"null pointer" in l.gdr_last_error()
    assert fn(C.byref(w), p, p, 2, 16, 4, 10, 0.8, 4, None, None, p, None, None, None, None, C.c_void_p(4096), 1 << 44, None) == _ffi.GDR_EINVAL
    assert b"null pointer" in l.gdr_last_error()


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_the_search_answers_as_before_when_out_len_is_given(which):
    from gdr_amd import _ffi
    l, fns = _fns()
    fn, w = fns[which], _weights()
    # what the score mode accepts stays refused for a search ...
    assert _call(fn, w, lens=True, R=1, nret=1, scores=True) == _ffi.GDR_EINVAL           # greedy: no trace
    assert b"step_scores" in l.gdr_last_error() and b"num_beams=1" in l.gdr_last_error()
    assert _call(fn, w, lens=True, R=1025) == _ffi.GDR_EINVAL and b"num_beams=1025" in l.gdr_last_error()
    assert _call(fn, w, lens=True, R=4, lp=0.0) == _ffi.GDR_EINVAL and b"length_penalty" in l.gdr_last_error()
    wide = _weights(V=200)                                       # 1024 x 201 candidates per query: over the select's limit
    assert _call(fn, wide, lens=True, R=1024) == _ffi.GDR_EINVAL and b"candidates" in l.gdr_last_error()
    need = l.gdr_t5_generate_workspace_bytes(C.byref(wide), 2, 16, 1024, 10)
    assert _call(fn, wide, R=1024, nbytes=need - 1) == _ffi.GDR_ENOSPC      # ... which the score mode has no use for
    assert _call(fn, w, lens=True, R=4, nret=5) == _ffi.GDR_EINVAL and b"num_return_sequences=5" in l.gdr_last_error()
    # ... and what a search accepts reaches its workspace check with the same size, nret < num_beams and a greedy lp <= 0 included
    for R, nret, lp in ((4, 4, 0.8), (4, 2, 0.8), (1, 1, -1.0), (100, 100, 1.0)):
        need = l.gdr_t5_generate_workspace_bytes(C.byref(w), 2, 16, R, 10)
        assert _call(fn, w, lens=True, R=R, nret=nret, lp=lp, nbytes=need - 1) == _ffi.GDR_ENOSPC, (R, nret)
        assert int(l.gdr_last_error().decode().rsplit("required", 1)[1]) == need


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_row_queries_is_a_known_rerank_flag_and_its_neighbours_are_not(which):
    from gdr_amd import _ffi
    l = _ffi.lib()
    fn = (l.gdr_rerank_topk, l.gdr_rerank_topk_bf16)[which]
    assert _ffi.RERANK_ROW_QUERIES == 8 and (_ffi.RERANK_POSITIONS, _ffi.RERANK_CHUNKED) == (1, 2)
    with open(os.path.join(os.path.dirname(_ffi.__file__), "..", "include", "gdr_hip.h")) as f:
        assert "#define GDR_RERANK_ROW_QUERIES 8\n" in f.read()
    p, ws = C.c_void_p(256), C.c_void_p(4096)

    def call(flags, nbytes):
        return fn(p, p, 64, p, p, p, 2, 10, p, 3, 10, 0, p, p, 100, 0, 0, 1000, flags, ws, nbytes, None)
    # accepted, alone and with the other two: the call gets as far as the workspace check, whose sizes the flag does not change
    for flags in (8, 8 | _ffi.RERANK_POSITIONS, 8 | _ffi.RERANK_CHUNKED, 8 | 3):
        need = l.gdr_rerank_workspace_bytes(2, 8193 if flags & _ffi.RERANK_CHUNKED else 100)
        assert call(flags, 0) == _ffi.GDR_ENOSPC, (flags, l.gdr_last_error())
        assert int(l.gdr_last_error().decode().rsplit("required", 1)[1]) <= need
    for flags in (4, 16, 8 | 4, 8 | 16):
        assert call(flags, 1 << 40) == _ffi.GDR_EINVAL and b"unknown flags" in l.gdr_last_error(), flags
    assert l.gdr_abi_version() == 9


# ------------------------------------------------------------------------------------------------ the flags of stage 2
def _ns(**kw):
    return types.SimpleNamespace(num_return_sequences=4, **kw)


def test_the_three_unimplemented_query_embed_combinations_are_refused_before_anything_runs():
    from gdr_amd import _ffi, main as gmain
    from gdr_amd.config import GDRConfig, stage2_query_form, unsupported_variant
    from gdr_amd.modeling import GDRRetriever
    fused = ["--use_query_embed_decoder_special", "1"]                                   # with the default use_query_embed_encoder 1
    fused_avg = ["--use_query_embed_encoder", "1", "--use_query_embed_decoder_avg", "1"]
    none = ["--use_query_embed_encoder", "0"]
    for argv, word in ((fused, "fusion_layer"), (fused_avg, "fusion_layer"), (none, "--use_query_embed_encoder 0")):
        a = gmain.parsers_parser(["--mode", "eval"] + argv)
        assert word in unsupported_variant(a)
        with pytest.raises(SystemExit) as e:
            GDRConfig.from_args(a)
        assert word in str(e.value)
        with pytest.raises(SystemExit) as e:                     # the entry point stops before touching a GPU or a file
            gmain.main(["--mode", "eval"] + argv)
        assert word in str(e.value)
        with pytest.raises(_ffi.GdrError) as e:                  # and so does the retriever, before it looks at its model
            GDRRetriever(None, None, None, a)
        assert word in str(e.value)
    # the sharded retriever carries one query vector per query
    for flag in ("special", "avg"):
        argv = ["--use_query_embed_encoder", "0", "--use_query_embed_decoder_" + flag, "1"]
        a = gmain.parsers_parser(["--mode", "eval"] + argv)
        assert unsupported_variant(a) is None and stage2_query_form(a) == (flag, None)
        assert stage2_query_form(a, sharded=True)[0] is None and "sharded" in stage2_query_form(a, sharded=True)[1]
        with pytest.raises(SystemExit) as e:                     # before any rank is started
            gmain.main(["--mode", "eval", "--n_gpu", "2"] + argv)
        assert "sharded" in str(e.value)
        with pytest.raises(_ffi.GdrError) as e:
            GDRRetriever(None, None, None, a, sharded=object())
        assert "sharded" in str(e.value)
    both = gmain.parsers_parser(["--mode", "eval", "--use_query_embed_encoder", "0", "--use_query_embed_decoder_special", "1",
                                 "--use_query_embed_decoder_avg", "1"])
    assert stage2_query_form(both) == ("special", None)          # the reference's later assignment wins (main_models.py:1568-1571)


def test_a_namespace_without_the_flags_stays_on_the_encoder_cls_path():
    from gdr_amd import main as gmain
    from gdr_amd.config import stage2_query_form, unsupported_variant
    from gdr_amd.modeling import GDRRetriever
    assert stage2_query_form(_ns()) == ("encoder", None) and stage2_query_form(_ns(), sharded=True) == ("encoder", None)
    assert unsupported_variant(_ns()) is None
    assert stage2_query_form(gmain.parsers_parser(["--mode", "eval"])) == ("encoder", None)
    r = GDRRetriever(None, None, None, _ns())                    # what every existing caller passes: no flag at all
    assert r.query_form == "encoder"
    assert GDRRetriever(None, None, None, _ns(), sharded=types.SimpleNamespace(D=None)).query_form == "encoder"
    assert GDRRetriever(None, None, None, _ns(use_query_embed_encoder=0, use_query_embed_decoder_avg=1)).query_form == "avg"


# ------------------------------------------------------------------------------------------------ forced_ref on hand-written cases
def test_forced_ref_scores_by_hand():
    # V = 2, ml = 4, Vd = 8: position p owns tokens 2p + 2, 2p + 3; EOS = 1
    ids = np.array([[0, 2, 1, 0],        # EOS at 2: two terms, len 2
                    [0, 1, 0, 0],        # EOS at 1: one term, len 1
                    [0, 3, 4, 6],        # no EOS: three terms, len 4
                    [0, 5, 1, 0],        # token 5 is no live column of position 0: the masked logit
                    [0, 4, 1, 0]])       # nor is 4, the first digit token of position 1, one past position 0's last live digit
    assert forced_ref.first_eos(ids).tolist() == [2, 1, 4, 2, 2]
    lg = np.full((5, 3, 8), -1e9)
    for p in range(3):
        lg[:, p, [2 * p + 2, 2 * p + 3, 1]] = np.log([1.0, 2.0, 5.0])       # probabilities 1/8, 2/8, 5/8
    got = forced_ref.scores_from_logits(lg, ids, 0.5)
    ln = np.log
    want = [(ln(1 / 8) + ln(5 / 8)) / 2 ** 0.5, ln(5 / 8) / 1.0, (ln(2 / 8) + ln(1 / 8) + ln(1 / 8)) / 4 ** 0.5, None]
    np.testing.assert_allclose(got[:3], want[:3], rtol=1e-12)
    np.testing.assert_allclose(got[3:], [(-1e9 - ln(8.0) + ln(5 / 8)) / 2 ** 0.5] * 2, rtol=1e-12)
    assert forced_ref.scores_from_logits(lg, ids, 1.0)[0] == pytest.approx((ln(1 / 8) + ln(5 / 8)) / 2)


def test_forced_ref_planes_by_hand():
    ids = np.array([[0, 2, 1, 0], [0, 3, 4, 6], [0, 1, 0, 0], [0, 0, 5, 1]])    # the last row holds a PAD token before its EOS
    h = np.arange(4 * 4 * 2, dtype=np.float32).reshape(4, 4, 2) + 1.0
    trace, at_eos, mean = forced_ref.planes_from_hidden(h, ids)
    assert forced_ref.counted(ids).tolist() == [[True, True, True, False], [True] * 4, [True, True, False, False], [True, False, True, True]]
    assert np.array_equal(trace[:3, 0], h[0, :3]) and not trace[3, 0].any()
    assert np.array_equal(trace[:, 1], h[1]) and not at_eos[1].any()
    assert np.array_equal(trace[:2, 2], h[2, :2]) and not trace[2:, 2].any()
    assert np.array_equal(at_eos[0], h[0, 2]) and np.array_equal(at_eos[2], h[2, 1]) and np.array_equal(at_eos[3], h[3, 3])
    np.testing.assert_array_equal(mean[0], (h[0, 0] + h[0, 1] + h[0, 2]) / np.float32(3))
    np.testing.assert_array_equal(mean[1], (h[1, 0] + h[1, 1] + h[1, 2] + h[1, 3]) / np.float32(4))
    np.testing.assert_array_equal(mean[3], (h[3, 0] + h[3, 2] + h[3, 3]) / np.float32(3))
    assert mean.dtype == np.float32


def test_forced_ref_row_query_rerank_by_hand_and_against_the_one_query_oracle():
    from oracle import retrieval_ref
    rng = np.random.default_rng(3)
    D = rng.standard_normal((12, 4)).astype(np.float32)
    members, segs = [[0, 1, 2, 3], [4, 5, 6]], [[1, 0, 3], [2, 1, 0]]
    beam = np.array([[-0.1, -0.5, -0.9], [-0.2, -0.3, -2.0]], np.float32)
    q = rng.standard_normal((2, 4)).astype(np.float32)
    # every query's row repeated R times: the one-query oracle
    v, i = forced_ref.rerank_row_queries(np.repeat(q, 3, axis=0), D, members, segs, beam, [0.0, 1.0], 3)
    ref = retrieval_ref.rerank(torch.from_numpy(q), torch.from_numpy(D), members, segs, beam.tolist(), [0.0, 1.0], 3)
    for b in range(2):
        for a in range(2):
            np.testing.assert_allclose(v[b, a], ref[b][a][0].numpy(), rtol=1e-6, atol=1e-6)
            assert i[b, a].tolist() == ref[b][a][1].tolist()
    # distinct rows, by hand: candidate 0 of query 0 meets row 0, candidates 1..3 meet row 2 (segment 1 is empty)
    qr = rng.standard_normal((6, 4)).astype(np.float32)
    v, i = forced_ref.rerank_row_queries(qr, D, members, segs, beam, [0.0], 4)
    sims = {0: np.tanh(np.dot(qr[0].astype(np.float64), D[0])), **{c: np.tanh(np.dot(qr[2].astype(np.float64), D[c])) for c in (1, 2, 3)}}
    order = sorted(sims, key=lambda c: -sims[c])
    assert i[0, 0].tolist() == order
    np.testing.assert_allclose(v[0, 0], [sims[c] for c in order], rtol=1e-12)
    assert i[1, 0, 3] == -1 and v[1, 0, 3] == -np.inf            # three candidates, k = 4
