"""Shared by tests/test_plain_head_host.py, tests/test_gpu_plain_head.py and tests/golden/make_golden_plain_head.py: the restatement
of the reference's ADAPTOR-FREE decode (`--adaptor_decode 0 --adaptor_efficient 0`: no adaptor is built, modeling_t5.py:1245-1249, and
the head is lm_head(sequence_output), :1640-1641) from pieces of the CPU oracle that are only imported, the cases the tests run with
the CPU-chosen seeds they rely on, and the zero-adaptor_linear twin of a plain model (the second yardstick: the shipped adaptor path
with adaptor_linear.weight = 0 computes the same head, 0 + e == e).  No test lives here."""
import functools

import numpy as np
import torch

import greedy_ref
from gdr_amd import synth
from gdr_amd.config import GDRConfig
from oracle import beam_ref, t5_ref

torch.set_grad_enabled(False)

GAP = greedy_ref.GAP        # 1e-3: ten times the project's fp32 tolerance 1e-4 + 1e-4*|ref|
SD_SEED = greedy_ref.SD_SEED
LIVE = -1e8                 # a ranked score above this belongs to a live beam (dead beams start at -1e9, generation_utils.py:663-668)


# ---------------------------------------------------------------------------------------------------------------- configs
def tiny(**over):
    return GDRConfig.tiny(adaptor_decode=0, adaptor_efficient=0, **over)


def base(**over):
    return GDRConfig.base(adaptor_decode=0, adaptor_efficient=0, **over)


def base2(**over):
    """t5-base widths with two encoder and two decoder blocks."""
    return base(num_layers=2, num_decoder_layers=2, **over)


def small2(**over):
    """The `--model_info small` widths (d = 512, 8 heads, d_ff 2048) with two blocks per stack."""
    return base(d_model=512, d_ff=2048, num_heads=8, num_layers=2, num_decoder_layers=2, **over)


def tiny8(**over):
    """The tiny shape with an adaptor_ff the bf16 linears take (every dim a multiple of 8) — for the adaptor twin of a bf16 case."""
    return tiny(adaptor_ff=128, **over)


def tiny_v30(**over):
    return tiny(output_vocab_size=30, decode_vocab_size=30 * 5 + 2, **over)        # 31 columns per position, Vd = 152


def tiny_v70(**over):
    return tiny(output_vocab_size=70, max_output_length=3, decode_vocab_size=70 * 3 + 2, **over)   # V + 1 = 71 > 64 columns


def wide(d, **over):
    """Tiny depth at another model width: 4 heads of d_kv = 16 inside d_model = d (the head kernel's pieces per lane follow d / 4)."""
    return tiny(d_model=d, **over)


CONFIGS = {"tiny": tiny, "base": base, "base2": base2, "small2": small2, "tiny8": tiny8, "tiny_v30": tiny_v30, "tiny_v70": tiny_v70,
           "d256": functools.partial(wide, 256), "d1024": functools.partial(wide, 1024), "d1280": functools.partial(wide, 1280)}


def with_adaptor(cfg):
    """The same shape with the adaptor head (what make_state_dict / T5DecoderHandle take for the zero-adaptor_linear twin)."""
    kw = cfg.to_dict()
    kw.update(adaptor_decode=1, adaptor_efficient=1)
    return GDRConfig(**kw)


@functools.lru_cache(maxsize=None)
def state_dict(kind, seed=SD_SEED):
    return synth.make_state_dict(CONFIGS[kind](), seed=seed)


def zero_adaptor_twin(kind, seed=SD_SEED, adaptor_layers=1):
    """(adaptor config, state dict): the plain model's weights plus a seeded adaptor whose adaptor_linear.weight is all zeros.  The
    adaptor has `adaptor_layers` layers (its output is multiplied by zero: one layer keeps the twin cheap)."""
    cfg = with_adaptor(CONFIGS[kind]())
    cfg.adaptor_layer_num = adaptor_layers
    sd = dict(state_dict(kind, seed))
    ad = synth_adaptor_only(cfg, seed + 1)
    ad["adaptor_linear.weight"] = torch.zeros((cfg.d_model * cfg.decode_vocab_size, cfg.d_model))
    sd.update(ad)
    return cfg, sd


def synth_adaptor_only(cfg, seed):
    """Seeded adaptor.* / adaptor_embeddings tensors of the shapes make_state_dict gives them (adaptor_linear is left to the caller:
    at t5-base it has 178 M entries, and the twin wants zeros)."""
    g = np.random.Generator(np.random.PCG64(seed))
    d, aff = cfg.d_model, cfg.adaptor_ff
    u = lambda shape, b: torch.from_numpy(((g.random(shape, dtype=np.float32) * 2.0 - 1.0) * np.float32(b)))   # noqa: E731
    sd = {}
    for i in range(cfg.adaptor_layer_num):
        p = f"adaptor.layers.{i}"
        for a in ("self_attn", "multihead_attn"):
            sd[f"{p}.{a}.in_proj_weight"], sd[f"{p}.{a}.in_proj_bias"] = u((3 * d, d), (1.5 / d) ** 0.5), u((3 * d,), 0.02)
            sd[f"{p}.{a}.out_proj.weight"], sd[f"{p}.{a}.out_proj.bias"] = u((d, d), d ** -0.5), u((d,), 0.02)
        sd[f"{p}.linear1.weight"], sd[f"{p}.linear1.bias"] = u((aff, d), d ** -0.5), u((aff,), d ** -0.5)
        sd[f"{p}.linear2.weight"], sd[f"{p}.linear2.bias"] = u((d, aff), aff ** -0.5), u((d,), aff ** -0.5)
        for n in ("norm1", "norm2", "norm3"):
            sd[f"{p}.{n}.weight"], sd[f"{p}.{n}.bias"] = 1.0 + u((d,), 0.1), u((d,), 0.05)
    sd["adaptor_embeddings"] = torch.from_numpy(g.random((1, 1, d), dtype=np.float32))
    return sd


# ---------------------------------------------------------------------------------------------------------------- the restatement
def all_logits(sd, cfg, dec_ids, enc_hidden, enc_mask):
    """The decode branch at every position (modeling_t5.py:1529-1576, :1640-1646 with no adaptor): [R, t, Vd].  The head dot is fp32
    also under t5_ref.bf16_linears() — include/gdr_hip.h keeps it so in the bf16 mode."""
    h = t5_ref.decoder_forward(sd, cfg, dec_ids, enc_hidden, enc_mask)
    t = dec_ids.shape[1]
    lg = (h * (cfg.d_model ** -0.5)) @ sd["lm_head.weight"].T
    return lg + t5_ref.positional_mask(t, cfg.decode_vocab_size, cfg.output_vocab_size, lg.dtype)[None]


def step_logits(sd, cfg, seq, enc_hidden, enc_mask):
    """Next-token logits [R, Vd] of the last position."""
    h = t5_ref.decoder_forward(sd, cfg, seq, enc_hidden, enc_mask)[:, -1]
    t = seq.shape[1]
    lg = (h * (cfg.d_model ** -0.5)) @ sd["lm_head.weight"].T
    return lg + t5_ref.positional_mask(t, cfg.decode_vocab_size, cfg.output_vocab_size, lg.dtype)[t - 1]


def beam_generate(sd, cfg, input_ids, attention_mask, num_beams, max_length=None, length_penalty=0.8, num_return_sequences=None,
                  trace=None, prefix_trace=None, decode_tree=None, enc_hidden=None):
    """generate() with beams over the restatement: ((decoded, scores), encoder states [B, L, d])."""
    B, R = attention_mask.shape[0], num_beams
    enc = t5_ref.encoder_forward(sd, cfg, input_ids, attention_mask) if enc_hidden is None else enc_hidden
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x, mask_x = enc.index_select(0, idx), attention_mask.index_select(0, idx)
    out = beam_ref.beam_search(lambda seq: step_logits(sd, cfg, seq, enc_x, mask_x), B, R, cfg.decode_vocab_size,
                               max_length or cfg.max_output_length, length_penalty, num_return_sequences or R, cfg.eos_token_id,
                               cfg.pad_token_id, cfg.decoder_start_token_id, trace=trace, decode_tree=decode_tree,
                               prefix_trace=prefix_trace)
    return out, enc


def greedy_generate(sd, cfg, input_ids, attention_mask, max_length=None, trace=None, enc_hidden=None):
    """generate() at num_beams = 1 over the restatement: (ids int64[B, width], sent_lengths)."""
    enc = t5_ref.encoder_forward(sd, cfg, input_ids, attention_mask) if enc_hidden is None else enc_hidden
    return greedy_ref.greedy_search(lambda seq: step_logits(sd, cfg, seq, enc, attention_mask), enc.shape[0],
                                    max_length or cfg.max_output_length, cfg.eos_token_id, cfg.pad_token_id,
                                    cfg.decoder_start_token_id, trace=trace)


def beam_min_gap(step_scores, final_scores, B, nret):
    """The seed rule's number: the smallest difference between adjacent live scores (> LIVE) of any step's ranked top-2R and between
    adjacent final scores of a query.  step_scores: iterable of [B, 2R] arrays; final_scores: B * nret values, query-major."""
    gap = np.inf
    for s in step_scores:
        s = np.asarray(s, dtype=np.float64)
        for b in range(s.shape[0]):
            live = s[b][s[b] > LIVE]
            if live.size > 1:
                gap = min(gap, float(np.min(-np.diff(live))))
    f = np.asarray(final_scores, dtype=np.float64).reshape(B, nret)
    f = np.where(f > LIVE, f, np.nan)
    if nret > 1:
        d = -np.diff(f, axis=1)
        if np.isfinite(d).any():
            gap = min(gap, float(np.nanmin(d)))
    return gap


# ---------------------------------------------------------------------------------------------------------------- the golden cases
# tests/golden/make_golden_plain_head.py runs the REFERENCE with both flags 0 on these; a case advances its token seed from 1 until
# the reference's own run clears GAP (beam_min_gap / greedy_ref's top-2 gap); g19 stores the seed taken and the gap.
GOLDEN_BEAM = {"tiny": ("tiny", 3, 8, 4, 0.8, 2), "base": ("base", 2, 40, 10, 0.8, 8)}      # kind, B, L, beams, length penalty, min_len
GOLDEN_GREEDY = ("tiny", 3, 8, 2)                                                         # kind, B, L, min_len


def golden_tokens(kind, B, L, min_len, seed):
    cfg = CONFIGS[kind]()
    return synth.make_tokens(B, L=L, vocab_hi=min(cfg.vocab_size, 32100), seed=seed, min_len=min_len)


# ---------------------------------------------------------------------------------------------------------------- the oracle cases
# Held to the restatement on the GPU: name -> (config, B, beams, L, token seed, min_len).  The seeds were picked on the CPU by
# `make_golden_plain_head.py --seeds`: the first from 1 on at which the restatement's own run clears GAP; test_plain_head_host.py
# asserts it again.  "trie": the constraint over TRIE_DOCS random docids (decode_tree=).
ORACLE_CASES = {
    "b1_r2_l3": ("tiny", 1, 2, 3, 1, 1),
    "b5_r6_l9": ("tiny", 5, 6, 9, 9, 2),
    "b2_r16_l12": ("tiny", 2, 16, 12, 356, 2),
    "l200": ("tiny", 2, 4, 200, 5, 100),
    "ragged": ("tiny", 5, 4, 12, 2, 1),
    "trie": ("tiny", 3, 4, 8, 1, 2),
}
TRIE_DOCS, TRIE_SEED = 20, 77
BF16_CASE = ("tiny8", 4, 4, 9, 6, 3)            # against the restatement under t5_ref.bf16_linears(), rule hypothesis_lists_match
BF16_BOUND = greedy_ref.BF16_GAP                # 5e-3


def trie_docids(cfg):
    """TRIE_DOCS distinct random docids of max_output_length - 2 digits (so EOS fits), as "a-b-c" strings."""
    g = np.random.Generator(np.random.PCG64(TRIE_SEED))
    depth, V = cfg.max_output_length - 2, cfg.output_vocab_size
    seen = []
    while len(seen) < TRIE_DOCS:
        s = "-".join(str(int(x)) for x in g.integers(0, V, size=depth))
        if s not in seen:
            seen.append(s)
    return seen


def docid_tokens(name, V):
    """"a-b-c" -> decoder tokens [a + 2, V + b + 2, 2V + c + 2, EOS] (position p owns tokens p*V + 2 ..)."""
    return [p * V + 2 + int(x) for p, x in enumerate(name.split("-"))] + [1]


def case_inputs(name, seed=None):
    kind, B, R, L, tok_seed, min_len = ORACLE_CASES[name] if name != "bf16" else BF16_CASE
    cfg = CONFIGS[kind]()
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=tok_seed if seed is None else seed, min_len=min_len)
    return cfg, state_dict(kind), ids, mask, R


def run_oracle(name, seed=None):
    """((decoded, scores), trace, prefix_trace, enc, gap) of a case over the restatement."""
    cfg, sd, ids, mask, R = case_inputs(name, seed)
    tree = beam_ref.build_trie([docid_tokens(n, cfg.output_vocab_size) for n in trie_docids(cfg)]) if name == "trie" else None
    trace, ptrace = [], []
    out, enc = beam_generate(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask), R, trace=trace, prefix_trace=ptrace,
                             decode_tree=tree)
    gap = beam_min_gap([s.numpy() for s, _ in trace], out[1], ids.shape[0], R)
    return out, trace, ptrace, enc, gap


@functools.lru_cache(maxsize=None)
def oracle(name):
    return run_oracle(name)
