#!/usr/bin/env python3
"""Generate tests/golden/g19_generate_plain.npz by running the REFERENCE's T5ForConditionalGeneration built with
adaptor_decode = 0 and adaptor_efficient = 0 (build container only, like make_golden.py, whose import shims and helpers it uses) on
this repo's seeded synthetic weights WITHOUT adaptor keys.  Arrays only: token batches, what generate() returned with 4 / 10 beams and
at its default num_beams = 1, the per-step top-2R trace, and the decode branch's logits at every position of one tiny batch.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plain_head.py            # writes g19_generate_plain.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plain_head.py --seeds    # prints the token seeds of plain_head_ref.ORACLE_CASES
    ... --base-from N    # resume the t5-base case's search at token seed N (the seeds below N were run before and did not clear)

A case moves on to the next token seed until, in the reference's own run, every adjacent pair of live scores in each step's top-2R and
every adjacent pair of a query's final scores (greedy: every deciding step's top-2 logits) differs by at least plain_head_ref.GAP; the
seed taken and the smallest gap are stored.  At t5-base widths random weights give nearly flat log-probabilities, so the 10-beam case
clears the rule about once in a few thousand seeds (a second per seed): --base-from resumes that search.  --seeds needs no reference: it applies the same rule to the restatement over the CPU oracle.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import make_golden as mg            # noqa: E402
import make_golden_greedy as mgg    # noqa: E402
import plain_head_ref as ph         # noqa: E402


def ref_t5_plain(cfg, sd):
    """The reference model with both adaptor flags 0 (main_models.py:748-780 forwards them into T5Config): it builds no adaptor and
    must load the adaptor-free state dict with no key missing or unexpected."""
    from transformers.configuration_t5 import T5Config
    from transformers.modeling_t5 import T5ForConditionalGeneration
    assert not cfg.has_adaptor and not any(k.startswith("adaptor") for k in sd)
    c = T5Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff, num_layers=cfg.num_layers,
                 num_decoder_layers=cfg.num_decoder_layers, num_heads=cfg.num_heads,
                 relative_attention_num_buckets=cfg.relative_attention_num_buckets, dropout_rate=0.1,
                 layer_norm_epsilon=cfg.layer_norm_epsilon, decode_embedding=2, decode_vocab_size=cfg.decode_vocab_size,
                 output_vocab_size=cfg.output_vocab_size, adaptor_decode=0, adaptor_efficient=0,
                 adaptor_layer_num=cfg.adaptor_layer_num, tie_decode_embedding=1, tie_word_embeddings=0, Rdrop=0.1, Rdrop_loss="KL",
                 Rdrop_only_decoder=0, denoising=0, multiple_decoder=0, decoder_num=1, max_output_length=cfg.max_output_length,
                 embedding_distillation=0.0, weight_distillation=0.0, decoder_start_token_id=0, hierarchic_decode=0, pad_token_id=0,
                 eos_token_id=1)
    with contextlib.redirect_stdout(io.StringIO()):
        m = T5ForConditionalGeneration(c)
    assert not any(k.startswith("adaptor") for k in m.state_dict()), "the reference built an adaptor although both flags are 0"
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all("denoising" in k for k in missing), missing
    return m.eval()


def _beam_case(name, first=1, limit=20000):
    kind, B, L, R, lp, min_len = ph.GOLDEN_BEAM[name]
    cfg, sd = ph.CONFIGS[kind](), ph.state_dict(kind)
    m = ref_t5_plain(cfg, sd)
    for seed in range(first, limit):
        ids, mask = ph.golden_tokens(kind, B, L, min_len, seed)
        outs, scores, enc, steps = mg._generate(m, torch.from_numpy(ids), torch.from_numpy(mask), cfg, R=R, lp=lp)
        gap = ph.beam_min_gap([s.numpy() for s, _ in steps], scores, B, R)
        print(f"beam {name}: seed {seed}, {len(steps)} steps, smallest gap {gap:.3e}", flush=True)
        if gap >= ph.GAP:
            break
    else:
        raise SystemExit(f"beam {name}: no seed below {limit} clears {ph.GAP}")
    a = {"input_ids": ids.astype(np.int16), "attention_mask": mask.astype(np.int8), "decoded": outs.numpy().astype(np.int16),
         "scores": np.array(scores, np.float64), "step_scores": torch.stack([s for s, _ in steps]).numpy(),
         "step_tokens": torch.stack([t for _, t in steps]).numpy().astype(np.int32), "num_beams": R, "length_penalty": lp,
         "token_seed": seed, "min_gap": gap}
    if name == "tiny":
        a["enc"] = enc[::R].numpy()                    # the reference hands the states back expanded per beam
    else:
        a["pooled"] = enc[::R, 0].numpy()
    return {f"{name}_{k}": v for k, v in a.items()}


def _greedy_case(limit=50):
    kind, B, L, min_len = ph.GOLDEN_GREEDY
    cfg, sd = ph.CONFIGS[kind](), ph.state_dict(kind)
    m = ref_t5_plain(cfg, sd)
    ml = cfg.max_output_length
    for seed in range(1, limit):
        ids, mask = ph.golden_tokens(kind, B, L, min_len, seed)
        out, steps = mgg._generate(m, torch.from_numpy(ids), torch.from_numpy(mask), cfg, ml)
        width = out.shape[1]
        chosen, smallest = np.zeros((width - 1, B), np.float32), np.inf
        for s, lg in enumerate(steps):
            top2 = torch.topk(lg, 2, dim=-1).values
            chosen[s] = top2[:, 0].numpy()
            unfinished = ~(out[:, 1:s + 1] == cfg.eos_token_id).any(dim=1).numpy()
            smallest = min(smallest, float((top2[:, 0] - top2[:, 1]).numpy()[unfinished].min()))
        print(f"greedy: seed {seed}, width {width}, smallest deciding gap {smallest:.3e}", flush=True)
        if smallest >= ph.GAP:
            break
    else:
        raise SystemExit(f"greedy: no seed below {limit} clears {ph.GAP}")
    return {"greedy_input_ids": ids.astype(np.int16), "greedy_attention_mask": mask.astype(np.int8), "greedy_ids": out.numpy().astype(np.int16),
            "greedy_chosen": chosen, "greedy_token_seed": seed, "greedy_min_gap": smallest, "greedy_max_length": ml}


def _logits_case():
    """g8 style: the decode branch's logits at every position for one tiny batch of digit prefixes."""
    cfg, sd = ph.tiny(), ph.state_dict("tiny")
    m = ref_t5_plain(cfg, sd)
    ids, mask = ph.golden_tokens("tiny", 3, 8, 2, 3)
    V, t = cfg.output_vocab_size, 4
    g = np.random.Generator(np.random.PCG64(9))
    dec = np.zeros((3, t), dtype=np.int64)
    for p in range(1, t):
        dec[:, p] = (p - 1) * V + 2 + g.integers(0, V, size=3)
    ids_t, mask_t = torch.from_numpy(ids), torch.from_numpy(mask)
    with torch.no_grad():
        enc = m.get_encoder()(ids_t, attention_mask=mask_t, return_dict=True)
        out = m(decoder_input_ids=torch.from_numpy(dec), encoder_outputs=enc, attention_mask=mask_t, use_cache=False, return_dict=True)
    return {"logits_input_ids": ids.astype(np.int16), "logits_attention_mask": mask.astype(np.int8),
            "logits_decoder_input_ids": dec.astype(np.int16), "logits": out.logits.numpy(), "logits_enc": enc.last_hidden_state.numpy()}


def g_generate_plain(base_from=1):
    mg.import_reference()
    arrays = {}
    arrays.update(_logits_case())
    arrays.update(_greedy_case())
    for name in ph.GOLDEN_BEAM:
        arrays.update(_beam_case(name, first=base_from if name == "base" else 1))
    mg.save("g19_generate_plain", seed=ph.SD_SEED, **arrays)


def pick_seeds(limit=5000):
    for name in ph.ORACLE_CASES:
        for seed in range(1, limit):
            gap = ph.run_oracle(name, seed)[4]
            if gap >= ph.GAP:
                print(f"{name}: seed {seed} (smallest gap {gap:.3e})", flush=True)
                break
        else:
            print(f"{name}: no seed below {limit}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", action="store_true")
    ap.add_argument("--base-from", type=int, default=1)
    a = ap.parse_args()
    pick_seeds() if a.seeds else g_generate_plain(a.base_from)
