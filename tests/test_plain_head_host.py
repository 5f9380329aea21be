"""The host side of the adaptor-free model (`--adaptor_decode 0 --adaptor_efficient 0`: the docid head is lm_head alone,
csrc/decode.hip head_plain_kernel): the restatement tests/plain_head_ref.py against what the reference itself returned with both
flags 0 (g19), the statements the GPU tests rely on about their CPU-chosen seeds, the config / CLI / synthetic-weights surface, and the
argument checks of the C entry points and the Python classes, which come before any launch and before any pointer is dereferenced —
no GPU needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import plain_head_ref as ph
from conftest import golden
from gdr_amd import synth
from gdr_amd.config import GDRConfig

torch.set_grad_enabled(False)
TOL = 1e-4


def _close(got, ref):
    np.testing.assert_allclose(np.asarray(got), np.asarray(ref), rtol=TOL, atol=TOL)


# ------------------------------------------------------------------------------------------------ the restatement against g19
@pytest.mark.parametrize("name", list(ph.GOLDEN_BEAM))
def test_restatement_beam_search_gives_what_the_reference_returned(name):
    g = golden("g19_generate_plain")
    kind, B, L, R, lp, min_len = ph.GOLDEN_BEAM[name]
    cfg, sd = ph.CONFIGS[kind](), ph.state_dict(kind)
    ids, mask = ph.golden_tokens(kind, B, L, min_len, int(g[f"{name}_token_seed"]))
    assert np.array_equal(ids, g[f"{name}_input_ids"]) and np.array_equal(mask, g[f"{name}_attention_mask"])
    assert int(g["seed"]) == ph.SD_SEED and int(g[f"{name}_num_beams"]) == R and float(g[f"{name}_length_penalty"]) == lp
    assert float(g[f"{name}_min_gap"]) >= ph.GAP                    # what the maker asserted of the reference's own scores
    ref_s, ref_t = g[f"{name}_step_scores"], g[f"{name}_step_tokens"]
    assert ph.beam_min_gap(ref_s, g[f"{name}_scores"], B, R) == pytest.approx(float(g[f"{name}_min_gap"]))
    trace = []
    (dec, sc), enc = ph.beam_generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), R, length_penalty=lp, trace=trace)
    assert np.array_equal(dec.numpy(), g[f"{name}_decoded"])
    _close(sc, g[f"{name}_scores"])
    assert len(trace) == ref_s.shape[0]
    ts, tt = np.stack([s.numpy() for s, _ in trace]), np.stack([t.numpy() for _, t in trace])
    live = ref_s > ph.LIVE
    _close(ts[live], ref_s[live])
    assert np.array_equal(tt[live], ref_t[live])
    if name == "tiny":
        _close(enc.numpy(), g["tiny_enc"])
    else:
        _close(enc[:, 0].numpy(), g["base_pooled"])


def test_restatement_greedy_search_gives_what_the_reference_returned():
    g = golden("g19_generate_plain")
    kind, B, L, min_len = ph.GOLDEN_GREEDY
    cfg, sd = ph.CONFIGS[kind](), ph.state_dict(kind)
    ids, mask = ph.golden_tokens(kind, B, L, min_len, int(g["greedy_token_seed"]))
    assert np.array_equal(ids, g["greedy_input_ids"]) and np.array_equal(mask, g["greedy_attention_mask"])
    assert float(g["greedy_min_gap"]) >= ph.GAP
    trace = []
    out, lens = ph.greedy_generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), int(g["greedy_max_length"]), trace=trace)
    ref = g["greedy_ids"]
    assert out.dtype == torch.int64 and tuple(out.shape) == ref.shape and np.array_equal(out.numpy(), ref)
    assert int(lens.max()) == ref.shape[1]
    _close(np.stack([c.numpy() for c, _, _ in trace]), g["greedy_chosen"])


def test_restatement_logits_at_every_position():
    g = golden("g19_generate_plain")
    cfg, sd = ph.tiny(), ph.state_dict("tiny")
    ids, mask = torch.from_numpy(g["logits_input_ids"].astype(np.int64)), torch.from_numpy(g["logits_attention_mask"].astype(np.int64))
    dec = torch.from_numpy(g["logits_decoder_input_ids"].astype(np.int64))
    from oracle import t5_ref
    enc = t5_ref.encoder_forward(sd, cfg, ids, mask)
    _close(enc.numpy(), g["logits_enc"])
    lg = ph.all_logits(sd, cfg, dec, enc, mask)
    ref = g["logits"]
    assert tuple(lg.shape) == ref.shape == (3, dec.shape[1], cfg.decode_vocab_size)
    np.testing.assert_allclose(lg.numpy(), ref, rtol=TOL, atol=TOL)
    assert (ref <= -1e8).sum() == 3 * dec.shape[1] * (cfg.decode_vocab_size - cfg.output_vocab_size - 1)   # the positional mask
    for t in range(1, dec.shape[1] + 1):                                                     # the step function is its last position
        _close(ph.step_logits(sd, cfg, dec[:, :t], enc, mask).numpy(), ref[:, t - 1])


@pytest.mark.parametrize("name", list(ph.ORACLE_CASES))
def test_committed_seeds_keep_their_margins(name):
    gap = ph.oracle(name)[4]
    print(f"{name}: smallest gap of the restatement {gap:.3e} (need >= {ph.GAP:g})")
    assert gap >= ph.GAP


def test_the_plain_head_equals_the_adaptor_head_with_a_zero_adaptor_linear():
    """The second yardstick, on the CPU oracle: t5_ref.decode_logits (decoder + adaptor + adaptor_linear head) with a zero
    adaptor_linear gives the restatement's logits — 0 + e == e."""
    from oracle import t5_ref
    cfg_p, sd_p = ph.tiny(), ph.state_dict("tiny")
    cfg_a, sd_a = ph.zero_adaptor_twin("tiny", adaptor_layers=2)
    assert cfg_a.has_adaptor and not cfg_p.has_adaptor
    ids, mask = synth.make_tokens(3, L=8, vocab_hi=cfg_p.vocab_size, seed=3, min_len=2)
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    enc = t5_ref.encoder_forward(sd_p, cfg_p, ids, mask)
    seq = torch.tensor([[0, 3, 9], [0, 7, 8], [0, 2, 13]])
    for restricted in (False, True):
        a = t5_ref.decode_logits(sd_a, cfg_a, seq, enc, mask, restricted=restricted)
        torch.testing.assert_close(a, ph.step_logits(sd_p, cfg_p, seq, enc, mask), rtol=TOL, atol=TOL)   # another summation order


# ------------------------------------------------------------------------------------------------ config, CLI, synthetic weights
def test_the_flag_pair_is_a_supported_variant_and_each_flag_alone_is_not():
    from gdr_amd import main as gmain
    from gdr_amd.config import unsupported_variant
    pair = ["--adaptor_decode", "0", "--adaptor_efficient", "0"]
    a = gmain.parsers_parser(["--mode", "eval"] + pair)
    assert unsupported_variant(a) is None
    cfg = GDRConfig.from_args(a)
    assert (cfg.adaptor_decode, cfg.adaptor_efficient, cfg.has_adaptor) == (0, 0, False)
    cfg = GDRConfig.from_args(gmain.parsers_parser(["--mode", "eval"]))
    assert (cfg.adaptor_decode, cfg.adaptor_efficient, cfg.has_adaptor) == (1, 1, True)
    for flag in ("adaptor_decode", "adaptor_efficient"):
        a = gmain.parsers_parser(["--mode", "eval", "--" + flag, "0"])
        why = unsupported_variant(a)
        assert why and "--" + flag in why and "--adaptor_decode 0 --adaptor_efficient 0" in why, why
        with pytest.raises(SystemExit) as e:
            GDRConfig.from_args(a)
        assert "--" + flag in str(e.value)
    # the pair does not excuse another refused flag
    why = unsupported_variant(gmain.parsers_parser(["--mode", "eval", "--position", "0"] + pair))
    assert why and "--position" in why


def test_a_half_set_config_is_a_value_error():
    for kw in (dict(adaptor_decode=0), dict(adaptor_efficient=0), dict(adaptor_decode=1, adaptor_efficient=0)):
        with pytest.raises(ValueError) as e:
            GDRConfig(**kw)
        assert "adaptor_decode" in str(e.value) and "adaptor_efficient" in str(e.value)
        with pytest.raises(ValueError):
            GDRConfig.tiny(**kw)
    assert GDRConfig().has_adaptor and GDRConfig.tiny().has_adaptor and GDRConfig.base().has_adaptor
    assert not GDRConfig.base(adaptor_decode=0, adaptor_efficient=0).has_adaptor
    assert not GDRConfig.tiny(adaptor_decode=0, adaptor_efficient=0).has_adaptor


def test_synthetic_weights_without_the_adaptor_are_the_same_draws():
    full = synth.make_state_dict(GDRConfig.tiny(), seed=1234)
    plain = synth.make_state_dict(ph.tiny(), seed=1234)
    assert not any(k.startswith("adaptor") for k in plain)
    assert set(plain) == {k for k in full if not k.startswith("adaptor")} and len(plain) < len(full)
    for k, v in plain.items():
        assert torch.equal(v, full[k]), k
    enc_only = synth.make_state_dict(ph.tiny(), seed=1234, with_decoder=False)
    assert all(torch.equal(v, full[k]) for k, v in enc_only.items())


# ------------------------------------------------------------------------------------------------ the C entry points
FAKE = 0x7f0000000000                          # a non-null "device" pointer: the host code must never dereference it


def _weights(plain, V=30, max_out_len=10, layers=2, **over):
    from gdr_amd import _ffi
    dl = (_ffi.GdrT5DecLayer * layers)()
    for ly in dl:
        for f, _t in ly._fields_:
            setattr(ly, f, FAKE)
    alr = (_ffi.GdrAdaptorLayer * 1)()
    for f, _t in alr[0]._fields_:
        setattr(alr[0], f, FAKE)
    dims = _ffi.GdrT5Dims(V * max_out_len + 2, 768, 64, 3072, 12, layers, 32, 128, 1e-6)
    if plain:
        w = _ffi.GdrT5DecoderWeights(dims, V, max_out_len, 0, 0, 0, 0.0, FAKE, FAKE, FAKE, FAKE, dl, None, None, FAKE)
    else:
        w = _ffi.GdrT5DecoderWeights(dims, V, max_out_len, 1, 8, 2048, 1e-5, FAKE, FAKE, FAKE, FAKE, dl, alr, FAKE, FAKE)
    for k, v in over.items():
        setattr(w, k, alr if v == "alayers" else v)
    w._keep = (dl, alr)
    return w


def _call(fn, w, B=2, L=16, R=4, ml=10, nret=None, nbytes=1 << 44, table=False):
    from gdr_amd import _ffi
    p = C.c_void_p(256)                                            # never dereferenced: every call here is refused first
    tab = None
    if table:
        tab = _ffi.GdrPrefixTable(FAKE, 10, w.out_vocab, 5, FAKE, FAKE, 1)
    return fn(C.byref(w), p, p, B, L, R, ml, 0.8, R if nret is None else nret, None, C.byref(tab) if tab is not None else None, p, p, p,
              None, None, C.c_void_p(4096), nbytes, None)


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_plain_weights_are_accepted_and_mixtures_are_refused_by_name(which):
    from gdr_amd import _ffi
    l = _ffi.lib()
    fn = (l.gdr_t5_generate, l.gdr_t5_generate_bf16)[which]
    # an accepted call gets as far as the workspace check: the dims check that divides by adaptor_nhead (0 here) is not run
    for R in (1, 4, 300):
        w = _weights(True)
        need = l.gdr_t5_generate_workspace_bytes(C.byref(w), 2, 16, R, 10)
        assert need > 0
        assert _call(fn, w, R=R, nbytes=need - 1) == _ffi.GDR_ENOSPC, l.gdr_last_error()
        assert int(l.gdr_last_error().decode().rsplit("required", 1)[1]) == need
    # adaptor_nhead / adaptor_ff / adaptor_eps are ignored for the plain form
    w = _weights(True, adaptor_nhead=7, adaptor_ff=13, adaptor_eps=3.0)
    assert l.gdr_t5_generate_workspace_bytes(C.byref(w), 2, 16, 4, 10) == l.gdr_t5_generate_workspace_bytes(C.byref(_weights(True)), 2, 16, 4, 10)
    assert _call(fn, w, nbytes=1) == _ffi.GDR_ENOSPC
    # partial combinations
    for over, name in ((dict(head_w=None), b"head_w"), (dict(alayers=None), b"alayers")):
        w = _weights(False, **over)
        assert _call(fn, w) == _ffi.GDR_EINVAL, over
        msg = l.gdr_last_error()
        assert name in msg and b"NULL" in msg and b"adaptor_layers=1" in msg, msg
    for over, name in ((dict(head_w=FAKE), b"head_w"), (dict(alayers="alayers"), b"alayers")):
        w = _weights(True, **over)
        assert _call(fn, w) == _ffi.GDR_EINVAL, over
        msg = l.gdr_last_error()
        assert name in msg and b"must be NULL" in msg and b"adaptor_layers=0" in msg, msg
    w = _weights(True, adaptor_layers=-1)
    assert _call(fn, w) == _ffi.GDR_EINVAL and b"adaptor_layers=-1" in l.gdr_last_error()
    w = _weights(True, head_e=None)
    assert _call(fn, w) == _ffi.GDR_EINVAL and b"null weight pointer" in l.gdr_last_error()
    # a prefix table with plain weights
    w = _weights(True)
    assert _call(fn, w, table=True) == _ffi.GDR_EINVAL
    msg = l.gdr_last_error()
    assert b"prefix_table" in msg and b"NULL" in msg and b"plain" in msg, msg
    # the adaptor form is what it was
    w = _weights(False)
    need = l.gdr_t5_generate_workspace_bytes(C.byref(w), 2, 16, 4, 10)
    assert _call(fn, w, nbytes=need - 1) == _ffi.GDR_ENOSPC


@pytest.mark.parametrize("which", [0, 1], ids=["f32", "bf16"])
def test_no_prefix_table_is_built_from_plain_weights(which):
    from gdr_amd import _ffi
    l = _ffi.lib()
    build = (l.gdr_t5_prefix_table_build, l.gdr_t5_prefix_table_build_bf16)[which]
    w = _weights(True)
    assert l.gdr_t5_prefix_table_workspace_bytes(C.byref(w), 100) == 0
    assert l.gdr_t5_prefix_table_workspace_bytes(C.byref(_weights(False)), 100) > 0
    lo = (C.c_int32 * 3)(0, 1, 5)
    p = C.c_void_p(256)
    assert build(C.byref(w), 2, lo, p, p, p, p, C.c_void_p(4096), 1 << 40, None) == _ffi.GDR_EINVAL
    msg = l.gdr_last_error()
    assert b"prefix_table_build" in msg and b"plain" in msg, msg
    w = _weights(False, head_w=None)
    assert build(C.byref(w), 2, lo, p, p, p, p, C.c_void_p(4096), 1 << 40, None) == _ffi.GDR_EINVAL
    assert b"head_w" in l.gdr_last_error()


def test_plain_workspace_leaves_out_the_head_matrix_and_the_adaptor():
    from gdr_amd import _ffi
    l = _ffi.lib()
    V, d, B, R, L, ml = 30, 768, 64, 10, 40, 10
    wa, wp = _weights(False, layers=6), _weights(True, layers=6)
    wa.adaptor_layers = 1                                        # one adaptor layer: the smallest adaptor there is
    a = l.gdr_t5_generate_workspace_bytes(C.byref(wa), B, L, R, ml)
    p = l.gdr_t5_generate_workspace_bytes(C.byref(wp), B, L, R, ml)
    head_matrix = B * R * (V + 1) * d * 4
    print(f"workspace at {B} x {R}, L = {L}: adaptor {a} bytes, plain {p} bytes, head-matrix buffer {head_matrix}")
    assert p > 0 and a - p >= head_matrix
    one, two = (l.gdr_t5_generate_workspace_bytes(C.byref(wp), B, L, r, ml) for r in (1, 2))
    assert 0 < one <= two <= p
    for shape in ((1, 1, 1, 2), (3, 8, 4, 5), (2, 512, 1024, 10)):
        assert l.gdr_t5_generate_workspace_bytes(C.byref(wp), *shape) > 0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_prefix_trie_is_refused_on_an_adaptor_free_model():
    from gdr_amd import _ffi, codec
    from gdr_amd.modeling import GDRModel
    cfg = ph.tiny()
    trie = codec.Trie.from_docids(ph.trie_docids(cfg), cfg.output_vocab_size)
    with pytest.raises(_ffi.GdrError) as e:
        GDRModel(cfg, ph.state_dict("tiny"), "cuda:0", prefix_trie=trie)
    assert "prefix_trie" in str(e.value) and "adaptor" in str(e.value)
    with pytest.raises(_ffi.GdrError) as e:
        from gdr_amd import ops
        dec = object.__new__(ops.T5DecoderHandle)
        dec.cfg = cfg
        ops.PrefixTable(dec, trie, "cuda:0")
    assert "adaptor" in str(e.value)


def test_the_state_dict_must_match_the_config():
    from gdr_amd import _ffi, ops
    full = synth.make_state_dict(GDRConfig.tiny(), seed=1234)
    with pytest.raises(_ffi.GdrError) as e:                    # trained adaptor weights are never dropped silently
        ops.T5DecoderHandle(ph.tiny(), full, torch.device("cuda:0"))
    assert "adaptor" in str(e.value) and "adaptor-free" in str(e.value)
    assert any(repr(k) in str(e.value) for k in full if k.startswith("adaptor"))
    only_linear = dict(ph.state_dict("tiny"))
    only_linear["adaptor_linear.weight"] = full["adaptor_linear.weight"]
    with pytest.raises(_ffi.GdrError) as e:
        ops.T5DecoderHandle(ph.tiny(), only_linear, torch.device("cuda:0"))
    assert "'adaptor_linear.weight'" in str(e.value)
    with pytest.raises(_ffi.GdrError) as e:                    # ... and an adaptor config never runs without them (was: KeyError)
        ops.T5DecoderHandle(GDRConfig.tiny(), ph.state_dict("tiny"), torch.device("cuda:0"))
    assert "'adaptor_embeddings'" in str(e.value)
    no_linear = {k: v for k, v in full.items() if k != "adaptor_linear.weight"}
    with pytest.raises(_ffi.GdrError) as e:
        ops.T5DecoderHandle(GDRConfig.tiny(), no_linear, torch.device("cuda:0"))
    assert "'adaptor_linear.weight'" in str(e.value)


def test_the_cli_refuses_the_prefix_table_with_the_flag_pair(tmp_path):
    from gdr_amd import main as gmain
    argv = ["--mode", "eval", "--adaptor_decode", "0", "--adaptor_efficient", "0", "--res1_save_path", str(tmp_path / "res1.tsv")]
    with pytest.raises(SystemExit) as e:                       # before any GPU work, any rank and any file
        gmain.main(argv + ["--prefix_table", "1"])
    assert "--prefix_table" in str(e.value) and "--adaptor_decode 0 --adaptor_efficient 0" in str(e.value)
    assert not (tmp_path / "res1.tsv").exists()
