"""Shared by tests/test_t5_long_host.py, tests/test_gpu_t5_long.py and tests/golden/make_golden_t5_long.py: the configs, token batches
and generate() cases of the T5 query tower above 128 input tokens, the CPU oracle runs (made once per process) and the margin rule that
the committed seeds satisfy.  No test lives here."""
import functools

import numpy as np
import torch

from gdr_amd import synth
from gdr_amd.config import GDRConfig

torch.set_grad_enabled(False)

GAP = 1e-3          # ten times the generate tests' tolerance (1e-4): what every cut of the oracle's search must clear
SD_SEED = 1234


def t64():
    """Two heads of 64: the key-block attention forms at the smallest widths that reach them."""
    return GDRConfig(vocab_size=128, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2, num_decoder_layers=2,
                     output_vocab_size=6, max_output_length=5, decode_vocab_size=32, adaptor_layer_num=2, adaptor_ff=96)


def base2():
    """t5-base widths with two encoder and two decoder blocks (one adaptor layer: the CPU oracle stays cheap)."""
    cfg = GDRConfig.base()
    cfg.num_layers, cfg.num_decoder_layers, cfg.adaptor_layer_num = 2, 2, 1
    return cfg


# "t64_sharp": t64 with decoder.final_layer_norm.weight x HEAD_SHARP, which multiplies the head's logits (as tests/peaked.py sharpens
# them): the synthetic weights put 100 final hypotheses inside one unit of score, where no token batch keeps all 99 neighbours 1e-3
# apart (tens of thousands tried); a sharper head spreads them as a trained one does.
HEAD_SHARP = 6.0
CONFIGS = {"t64": t64, "t64_sharp": t64, "tiny": GDRConfig.tiny, "base2": base2}


@functools.lru_cache(maxsize=None)
def state_dict(kind, seed=SD_SEED):
    sd = synth.make_state_dict(CONFIGS[kind](), seed=seed)
    if kind == "t64_sharp":
        sd = dict(sd)
        sd["decoder.final_layer_norm.weight"] = sd["decoder.final_layer_norm.weight"] * HEAD_SHARP
    return sd


def tokens_with_lengths(lens, L, vocab, seed):
    """ids int64[B, L] uniform in [2, vocab), EOS(1) at the end of each sequence, PAD(0) behind; mask = prefix of ones."""
    g = np.random.Generator(np.random.PCG64(seed))
    lens = np.asarray(lens)
    ids = g.integers(2, vocab, size=(len(lens), L)).astype(np.int64)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    ids[np.arange(len(lens)), lens - 1] = 1
    return ids * mask, mask


# ---------------------------------------------------------------------------------------------------------------- generate() cases
# name -> (config, R, L, sequence lengths, max_length, token seed, trie: 0 = none, n = every n-th two-digit docid).  The token seeds were picked on the CPU by
# `tests/golden/make_golden_t5_long.py --seeds` as the first seed from 1 on whose oracle search clears GAP at every cut (margins());
# tests/test_t5_long_host.py asserts that for every row, and each GPU test asserts it again before it looks at the GPU.
GEN_CASES = {
    "t64_129": ("t64", 4, 129, (129, 70), 5, 1, 0),
    "t64_300": ("t64", 4, 300, (300, 140), 5, 1, 0),
    "t64_512": ("t64", 10, 512, (512, 140, 9), 5, 3, 0),
    "t64_200_r100": ("t64_sharp", 100, 200, (200,), 5, 28, 0),
    "t64_300_trie": ("t64", 4, 300, (300, 140), 5, 1, 3),
    "tiny_300": ("tiny", 4, 300, (300, 131), 5, 1, 0),
    "base2_512": ("base2", 4, 512, (512, 140), 6, 1, 0),
    "t64_200_step": ("t64", 4, 200, (200, 131, 17), 5, 1, 1),
}
# The 100-beam shape on the plain t64 weights as well, where the margin rule cannot hold (see HEAD_SHARP): held to the tie-aware rule
# of oracle/parity_rules.py instead of equal ids, so it is no row of GEN_CASES and assert_margins is not asked of it.
TIE_CASES = {
    "t64_200_r100_plain": ("t64", 100, 200, (200,), 5, 1, 0),
}


def trie_docids(V, every):
    """Every `every`-th two-digit docid over V symbols (every third: as __graft_entry__.smoke; every one: the full trie)."""
    return ["-".join(str(x) for x in synth.cluster_digits(c, 2, V)) for c in range(0, V * V, every)]


def case_inputs(name, seed=None):
    kind, R, L, lens, ml, tok_seed, use_trie = (GEN_CASES.get(name) or TIE_CASES[name])
    cfg = CONFIGS[kind]()
    ids, mask = tokens_with_lengths(lens, L, min(cfg.vocab_size, 32100), tok_seed if seed is None else seed)
    return cfg, state_dict(kind), ids, mask, R, ml, use_trie


def run_oracle(name, seed=None):
    """beam_ref.generate of a case with its per-step trace: (decoded int64, scores list, trace, prefix_trace, tree)."""
    from oracle import beam_ref, codec_ref, t5_ref
    cfg, sd, ids, mask, R, ml, use_trie = case_inputs(name, seed)
    tree = None
    if use_trie:
        V = cfg.output_vocab_size
        tree = beam_ref.build_trie([codec_ref.encode_single_newid(s, kary=V) for s in trie_docids(V, use_trie)])
    it, mt = torch.from_numpy(ids), torch.from_numpy(mask)
    B = ids.shape[0]
    enc = t5_ref.encoder_forward(sd, cfg, it, mt)
    idx = torch.arange(B).view(-1, 1).repeat(1, R).view(-1)
    enc_x, mask_x = enc.index_select(0, idx), mt.index_select(0, idx)
    trace, ptrace = [], []
    rd, rs = beam_ref.beam_search(lambda seq: t5_ref.decode_logits(sd, cfg, seq, enc_x, mask_x, restricted=True), B, R,
                                  cfg.decode_vocab_size, ml, 0.8, R, cfg.eos_token_id, cfg.pad_token_id, cfg.decoder_start_token_id,
                                  trace=trace, decode_tree=tree, prefix_trace=ptrace)
    return rd, rs, trace, ptrace, tree


@functools.lru_cache(maxsize=None)
def oracle(name):
    return run_oracle(name)


def margins(trace, scores, B, R, Vd, eos=1):
    """(smallest gap at a cut of the search, smallest gap between adjacent final scores of a query), over finite scores only.
    The cuts of a step (generation_utils.py:800-829) are: rank R-1 | R of the 2R ranked candidates (an EOS candidate counts only
    above it) and the R-th | (R+1)-th candidate that is not EOS (the beams that continue), where the trace's 2R candidates show both
    sides.  A cut whose upper side is a masked (-1e9) or trie-forbidden (-inf) candidate separates nothing that is returned."""
    step = np.inf
    for sc, tk in trace:
        sc, tk = sc.numpy().astype(np.float64), tk.numpy()
        for b in range(B):
            if sc[b, R - 1] > -1e8:
                step = min(step, sc[b, R - 1] - sc[b, R])
            non_eos = [i for i in range(2 * R) if tk[b, i] % Vd != eos]
            if len(non_eos) > R and sc[b, non_eos[R - 1]] > -1e8:
                step = min(step, sc[b, non_eos[R - 1]] - sc[b, non_eos[R]])
    fin = np.inf
    rs = np.asarray(scores, np.float64).reshape(B, R)
    for b in range(B):
        f = rs[b][np.isfinite(rs[b]) & (rs[b] > -1e8)]
        if len(f) > 1:
            fin = min(fin, float(np.min(-np.diff(f))))
    return float(step), float(fin)


def assert_margins(name):
    """The oracle's search of a committed case clears GAP at every cut and between adjacent final hypotheses."""
    cfg, _, ids, _, R, _, _ = case_inputs(name)
    rd, rs, trace, _, _ = oracle(name)
    step, fin = margins(trace, rs, ids.shape[0], R, cfg.decode_vocab_size)
    print(f"{name}: smallest cut gap {step:.3e}, smallest gap between adjacent final scores {fin:.3e} (need > {GAP:g})")
    assert step > GAP and fin > GAP, (name, step, fin)
    return rd, rs
