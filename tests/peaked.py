"""Inputs, references and recorded figures of the peaked-softmax cases: test_peaked_host.py checks them on the CPU; the GPU parity tests
of the same cases import them from here (shapes, weights, float64 references and bounds).

synth.make_state_dict follows the reference initialiser: the scores entering every softmax have a standard deviation of about 1, the
probabilities are close to uniform and the beam step ranks candidates half a unit apart.  A trained T5 has scores in the tens, relative
biases of several units and a sharply peaked docid head.  peaked_t5 / peaked_bert scale the synthesised weights into that range; the
reference every kernel is held to is the oracle in float64 (oracle/*.py follow the dtype of the state dict).

The case tables below hold, next to the shapes, what the host test measured once and re-asserts: `g` = max |oracle fp32 - oracle float64|
(the distance of one honest fp32 implementation from the truth on these inputs) and, for the bf16 mode, the distance between its emulation
with fp32 and with float64 accumulation.  The GPU bounds follow from these figures alone (fp32_bound), never from a kernel's output.
"""
import collections
import functools

import numpy as np
import torch

from gdr_amd import synth
from gdr_amd.config import GDRConfig

Setting = collections.namedtuple("Setting", "name s rb hs bert_s min_score")
MODERATE = Setting("moderate", 6.0, 30.0, 6.0, 6.0, 20.0)
STRONG = Setting("strong", 12.0, 60.0, 12.0, 20.0, 40.0)
SETTINGS = {"moderate": MODERATE, "strong": STRONG}
MIN_TOP_PROB = 0.5

CFG64 = dict(d_model=128, d_kv=64, num_heads=4, d_ff=256)


# ------------------------------------------------------------------------------------------------------------ weights
def peaked_t5(sd, cfg, s, rb, hs):
    """A new state dict: every *Attention.q.weight x s, every relative_attention_bias.weight x rb, the q rows of every adaptor
    in_proj_weight / in_proj_bias x s, decoder.final_layer_norm.weight x hs (it multiplies the head's logits)."""
    d, out = cfg.d_model, {}
    for k, v in sd.items():
        if k.endswith("Attention.q.weight"):
            v = v * s
        elif k.endswith("relative_attention_bias.weight"):
            v = v * rb
        elif k.endswith("in_proj_weight") or k.endswith("in_proj_bias"):
            v = v.clone()
            v[:d] *= s
        elif k == "decoder.final_layer_norm.weight":
            v = v * hs
        out[k] = v
    return out


def peaked_bert(sd, s):
    return {k: (v * s if "attention.self.query." in k else v) for k, v in sd.items()}


def as_float64(sd):
    return {k: v.to(torch.float64) for k, v in sd.items()}


def score_stats(scores):
    """scores: what enters a softmax, additive mask included.  Returns (max |unmasked score|, mean top probability over the rows that
    have at least two unmasked keys)."""
    sc = scores.double()
    rows = (sc > -1e8).sum(-1) >= 2
    return float(sc[sc > -1e8].abs().max()), float(torch.softmax(sc, -1).max(-1).values[rows].mean())


def t5_block0_scores(sd, cfg, ids, mask):
    """The scores of the encoder's block 0, restated from the oracle's own parts (t5_ref.encoder_forward, t5_attention)."""
    from oracle import t5_ref
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    B, L = ids.shape
    p = "encoder.block.0.layer.0."
    nx = t5_ref.t5_layer_norm(sd["shared.weight"][ids], sd[p + "layer_norm.weight"], cfg.layer_norm_epsilon)
    q, k = (t5_ref._lin(nx, sd[p + f"SelfAttention.{n}.weight"]).view(B, L, cfg.num_heads, cfg.d_kv).transpose(1, 2) for n in "qk")
    bias = t5_ref.compute_bias(L, L, sd[p + "SelfAttention.relative_attention_bias.weight"], True, cfg.relative_attention_num_buckets)
    return q @ k.transpose(3, 2) + bias + (1.0 - mask[:, None, None, :].to(nx.dtype)) * -1e9


def bert_block0_scores(sd, bc, ids, mask):
    """The scores of the doc tower's block 0, restated from bert_ref.bert_forward."""
    import torch.nn.functional as F
    from oracle.bert_ref import P as pre
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    B, L = ids.shape
    d, H = bc["hidden_size"], bc["num_heads"]
    e = pre + "embeddings."
    x = sd[e + "word_embeddings.weight"][ids] + sd[e + "position_embeddings.weight"][:L][None] + sd[e + "token_type_embeddings.weight"][0]
    x = F.layer_norm(x, (d,), sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], bc["eps"])
    a = pre + "encoder.layer.0.attention.self."
    q, k = ((x @ sd[a + n + ".weight"].T + sd[a + n + ".bias"]).view(B, L, H, d // H).permute(0, 2, 1, 3) for n in ("query", "key"))
    return q @ k.transpose(-1, -2) / (d // H) ** 0.5 + (1.0 - mask[:, None, None, :].to(x.dtype)) * -1e9


def decode_step0_stats(sd, cfg, ids, mask):
    """Peakedness of the decode chain at its first step (every beam row holds START): score_stats of decoder block 0's cross-attention
    over the oracle's encoder states, and the mean top probability of the head's distribution over the docid columns."""
    from oracle import t5_ref
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    B, L = ids.shape
    H, dk, eps = cfg.num_heads, cfg.d_kv, cfg.layer_norm_epsilon
    enc = t5_ref.encoder_forward(sd, cfg, ids, mask)
    start = torch.full((B, 1), cfg.decoder_start_token_id, dtype=torch.long)
    p = "decoder.block.0.layer."
    h = sd["decode_embeddings.weight"][start]
    nx = t5_ref.t5_layer_norm(h, sd[p + "0.layer_norm.weight"], eps)      # one key: the self-attention returns o(v(nx))
    h = h + t5_ref._lin(t5_ref._lin(nx, sd[p + "0.SelfAttention.v.weight"]), sd[p + "0.SelfAttention.o.weight"])
    nx = t5_ref.t5_layer_norm(h, sd[p + "1.layer_norm.weight"], eps)
    q = t5_ref._lin(nx, sd[p + "1.EncDecAttention.q.weight"]).view(B, 1, H, dk).transpose(1, 2)
    k = t5_ref._lin(enc, sd[p + "1.EncDecAttention.k.weight"]).view(B, L, H, dk).transpose(1, 2)
    bias = t5_ref.compute_bias(1, L, sd[p + "1.EncDecAttention.relative_attention_bias.weight"], True, cfg.relative_attention_num_buckets)
    cross = q @ k.transpose(3, 2) + bias + (1.0 - mask[:, None, None, :].to(h.dtype)) * -1e9
    logits = t5_ref.decode_logits(sd, cfg, start, enc, mask, restricted=True)
    return score_stats(cross), float(torch.softmax(logits.double(), -1).max(-1).values.mean())


def fp32_bound(g):
    """max(1e-4, 4 g): 1e-4 is the project's own tolerance; kernel and fp32 oracle are two fp32 sums in different orders, each about g
    from the float64 value (x 2), and the maximum is taken over other elements than the ones g was seen on (x 2)."""
    return max(1e-4, 4.0 * g)


def tokens_with_lengths(lens, L, vocab, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens)
    ids = g.integers(2, vocab, size=(len(lens), L)).astype(np.int64)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    ids[np.arange(len(lens)), lens - 1] = 1
    return ids * mask, mask


def tied_row_share(scores, tol):
    """Share of beam rows whose score lies within 2 tol of a neighbour's in the same query: the tie groups of hypothesis_lists_match,
    the id rule of the generate cases — the rows whose ids that rule does not compare position by position."""
    sc = np.asarray(scores, np.float64)
    near = np.abs(sc[:, :-1] - sc[:, 1:]) <= 2 * tol
    tied = np.zeros(sc.shape, bool)
    tied[:, :-1] |= near
    tied[:, 1:] |= near
    return float(tied.mean())


# ------------------------------------------------------------------------------------------------------------ case tables
# T5 encoder.  shapes: L -> sequence lengths (every case holds 1, 16, 17 and L).  g: recorded max |fp32 - float64| over hidden states.
_PACKED_LENS = (1, 16, 17, 48, 2, 7, 15, 23, 31, 32, 33, 40, 44, 47, 11, 26)
ENCODER_CASES = {
    "enc-generic": dict(cfg={}, seed=301, shapes={9: (1, 5, 9), 70: (16, 17, 70)}, g=dict(moderate=5.00e-6, strong=1.05e-5)),
    "enc-mfma": dict(cfg=CFG64, seed=302, shapes={17: (1, 16, 17, 9), 48: (1, 16, 17, 48), 128: (1, 16, 17, 128)},
                     g=dict(moderate=9.60e-6, strong=3.60e-5)),
    "enc-packed": dict(cfg=CFG64, seed=303, shapes={48: _PACKED_LENS}, g=dict(moderate=1.05e-5, strong=2.80e-5)),
}
# the bf16 mode on the enc-packed inputs: MODERATE with q x `s`; noise = |emulation fp32 sums - emulation float64 sums| (max, mean)
ENC_BF16 = dict(case="enc-packed", s=3.0, noise=(6.8e-3, 2.35e-4))

# doc tower.  B = 8, L = 100
_BERT_LENS = (1, 16, 17, 100, 50, 64, 65, 99)
BERT_CASES = {
    "bert-64": dict(bc={}, seed=311, L=100, lens=_BERT_LENS, g=dict(moderate=1.34e-5, strong=7.50e-5)),
    "bert-16": dict(bc=dict(num_heads=8), seed=312, L=100, lens=_BERT_LENS, g=dict(moderate=8.70e-6, strong=3.80e-5)),
}
# bert-bf16: the maximum (one flipped bf16 rounding carried through a LayerNorm) is 2.95e-2 at q x 6, 1.23e-2 at x 2 and still 1.02e-2 with
# the weights as synthesised, so no q scale brings 4 x max under the 3e-2 cap.  The case stays at MODERATE and is held to statistics that
# do meet the cap: p99 = the 99th percentile of the noise (4 x p99 = 2.5e-2), and over = the share of elements whose noise exceeds
# 3e-2 / 4 — at 4 x the noise at most that share of a kernel's elements may exceed 3e-2
BERT_BF16 = dict(case="bert-64", s=6.0, noise=(2.95e-2, 5.7e-4), p99=6.3e-3, over=6.5e-3)

# generate().  shape = (B queries, R beams, L); g: recorded max |fp32 - float64| over the final beam scores
GENERATE_CASES = {
    "gen-generic": dict(cfg={}, seed=321, shape=(5, 6, 9), g=dict(moderate=7.10e-6, strong=2.50e-5)),
    "gen-64": dict(cfg=CFG64, seed=322, shape=(8, 6, 20), g=dict(moderate=6.30e-6, strong=4.80e-5)),
    "gen-cross-mfma": dict(cfg=CFG64, seed=323, shape=(80, 20, 23), g=dict(moderate=2.20e-5, strong=3.60e-4)),
    "gen-heads4": dict(cfg=dict(CFG64, max_output_length=10, decode_vocab_size=62), seed=324, shape=(128, 32, 12),
                       g=dict(moderate=1.80e-5, strong=1.10e-4)),
    # 19 output positions: the decoder's and the adaptor's self-attention see 17 and 18 keys in the last two steps, more than the 16
    # attention_decode_short_kernel holds — attention_decode_rows_kernel
    "gen-rows": dict(cfg=dict(CFG64, max_output_length=19, decode_vocab_size=6 * 19 + 2), seed=325, shape=(4, 6, 11),
                     g=dict(moderate=4.00e-6, strong=2.50e-5)),
}
GEN_BF16 = dict(case="gen-64", s=6.0, noise=(7.3e-3, 8.3e-4))


# ------------------------------------------------------------------------------------------------------------ encoder
@functools.lru_cache(maxsize=None)
def encoder_case(name, setting):
    """(cfg, peaked fp32 state dict, {L: (ids, mask)})."""
    c = ENCODER_CASES[name]
    cfg = GDRConfig.tiny(**c["cfg"])
    sd = peaked_t5(synth.make_state_dict(cfg, seed=c["seed"], with_decoder=False), cfg, setting.s, setting.rb, setting.hs)
    inputs = {L: tokens_with_lengths(lens, L, cfg.vocab_size, c["seed"] * 1000 + L) for L, lens in c["shapes"].items()}
    return cfg, sd, inputs


@functools.lru_cache(maxsize=None)
def encoder_oracle(name, setting, f64, bf16=False):
    """{L: hidden states ndarray[B, L, d]} of the oracle: fp32 or float64 sums, optionally the bf16 mode's rounding points."""
    from oracle import t5_ref
    cfg, sd, inputs = encoder_case(name, setting)
    sd = as_float64(sd) if f64 else sd
    out = {}
    for L, (ids, mask) in inputs.items():
        if bf16:
            with t5_ref.bf16_linears():
                h = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask))
        else:
            h = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask))
        assert h.dtype == (torch.float64 if f64 else torch.float32)
        out[L] = h.numpy()
    return out


def bf16_setting(table):
    return MODERATE._replace(s=table["s"], bert_s=table["s"])


# ------------------------------------------------------------------------------------------------------------ doc tower
@functools.lru_cache(maxsize=None)
def bert_case(name, setting):
    c = BERT_CASES[name]
    bc = dict(synth.bert_config(True), **c["bc"])
    sd = peaked_bert(synth.make_bert_state_dict(bc, seed=c["seed"]), setting.bert_s)
    return bc, sd, tokens_with_lengths(c["lens"], c["L"], bc["vocab_size"], c["seed"] * 1000)


@functools.lru_cache(maxsize=None)
def bert_oracle(name, setting, f64, bf16=False):
    from oracle import bert_ref
    bc, sd, (ids, mask) = bert_case(name, setting)
    hid, _ = bert_ref.bert_forward(as_float64(sd) if f64 else sd, bc, torch.from_numpy(ids), torch.from_numpy(mask), bf16=bf16)
    assert hid.dtype == (torch.float64 if f64 else torch.float32)
    return hid.numpy()


# ------------------------------------------------------------------------------------------------------------ generate
@functools.lru_cache(maxsize=None)
def generate_case(name, setting):
    c = GENERATE_CASES[name]
    cfg = GDRConfig.tiny(**c["cfg"])
    sd = peaked_t5(synth.make_state_dict(cfg, seed=c["seed"]), cfg, setting.s, setting.rb, setting.hs)
    B, R, L = c["shape"]
    ids, mask = synth.make_tokens(B, L=L, vocab_hi=cfg.vocab_size, seed=c["seed"], min_len=2)
    return cfg, sd, ids, mask, R


@functools.lru_cache(maxsize=None)
def generate_oracle(name, setting, f64):
    """beam_ref.generate's search (encoder once, states expanded per beam, restricted head) in fp32 or float64:
    (hypothesis lists per query, scores ndarray[B, R], trace, prefix_trace)."""
    from oracle import beam_ref, t5_ref
    cfg, sd, ids, mask, R = generate_case(name, setting)
    sd = as_float64(sd) if f64 else sd
    B = ids.shape[0]
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x = t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask)).index_select(0, idx)
    mask_x = torch.from_numpy(mask).index_select(0, idx)
    trace, ptrace = [], []
    dec, sc = beam_ref.beam_search(lambda seq: t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True), B, R,
                                   cfg.decode_vocab_size, cfg.max_output_length, 0.8, R, trace=trace, prefix_trace=ptrace)
    return hypothesis_lists(dec.numpy(), B, R), np.array(sc, np.float64).reshape(B, R), trace, ptrace


@functools.lru_cache(maxsize=None)
def generate_bf16_encoder_states(setting):
    """The bf16 decode case isolates the decode chain: both sides start from the fp32 oracle's encoder states."""
    from oracle import t5_ref
    cfg, sd, ids, mask, R = generate_case(GEN_BF16["case"], setting)
    return t5_ref.encoder_forward(sd, cfg, torch.from_numpy(ids), torch.from_numpy(mask))


@functools.lru_cache(maxsize=None)
def generate_bf16_oracle(setting, f64):
    """The decode chain's bf16 emulation (t5_ref.bf16_linears) with fp32 or float64 sums on generate_bf16_encoder_states:
    (hypothesis lists per query, scores ndarray[B, R], trace, prefix_trace)."""
    from oracle import beam_ref, t5_ref
    cfg, sd, ids, mask, R = generate_case(GEN_BF16["case"], setting)
    B = ids.shape[0]
    enc = generate_bf16_encoder_states(setting)
    if f64:
        sd, enc = as_float64(sd), enc.double()
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x, mask_x = enc.index_select(0, idx), torch.from_numpy(mask).index_select(0, idx)

    def step(seq):
        with t5_ref.bf16_linears():
            return t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True)

    trace, ptrace = [], []
    dec, sc = beam_ref.beam_search(step, B, R, cfg.decode_vocab_size, cfg.max_output_length, 0.8, R, trace=trace, prefix_trace=ptrace)
    return hypothesis_lists(dec.numpy(), B, R), np.array(sc, np.float64).reshape(B, R), trace, ptrace


def hypothesis_lists(decoded, B, R):
    """Per query the R returned token rows as tuples without their trailing PAD (the width of `decoded` depends on the longest row)."""
    def strip(r):
        while r and r[-1] == 0:
            r.pop()
        return tuple(r)
    return [[strip(r) for r in decoded[b * R:(b + 1) * R].tolist()] for b in range(B)]


def shared_score_gaps(lists_a, scores_a, lists_b, scores_b):
    """|score_a - score_b| of every hypothesis both searches returned for the same query."""
    gaps = []
    for la, sa, lb, sb in zip(lists_a, scores_a, lists_b, scores_b):
        where = {x: i for i, x in enumerate(lb)}
        gaps += [abs(sa[p] - sb[where[x]]) for p, x in enumerate(la) if x in where]
    return np.array(gaps, np.float64)
