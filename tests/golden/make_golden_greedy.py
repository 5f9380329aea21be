#!/usr/bin/env python3
"""Generate tests/golden/g18_generate_greedy.npz by running the REFERENCE's generate() at its default num_beams = 1 (build container
only, like make_golden.py, whose import shims and helpers it uses) on the cases of tests/greedy_ref.GOLDEN_CASES, with this repo's
seeded synthetic weights.  Arrays only: token batches, the returned ids, and per step the chosen logit and the top-2 gap.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_greedy.py            # writes g18_generate_greedy.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_greedy.py --seeds    # prints the token seeds of greedy_ref.ORACLE_CASES

A case moves on to the next token seed until every step that decides a token has a top-2 gap >= greedy_ref.GAP in the reference
itself; the seed taken and the smallest gap are stored.  --seeds needs no reference: it applies the rules written beside
greedy_ref.ORACLE_CASES to the restatement over the CPU oracle.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import make_golden as mg      # noqa: E402
import greedy_ref             # noqa: E402


def _generate(m, ids_t, mask_t, cfg, max_length):
    """The reference's generate() with no beam arguments; torch.argmax is watched for the per-step logits."""
    steps = []
    orig = torch.argmax

    def spy(x, *a, **kw):
        r = orig(x, *a, **kw)
        if x.dim() == 2 and x.shape[1] == cfg.decode_vocab_size:
            steps.append(x.detach().clone())
        return r

    torch.argmax = spy
    try:
        with torch.no_grad():
            out, enc = mg.quiet(m.generate, ids_t, attention_mask=mask_t, use_cache=False, max_length=max_length, decode_embedding=2,
                                decode_vocab_size=cfg.decode_vocab_size, decode_tree=None, decoder_index=-1, cluster_constraint=None)
    finally:
        torch.argmax = orig
    assert torch.is_tensor(out) and enc is None
    return out, steps


def g_generate_greedy(limit=50):
    mg.import_reference()
    arrays = {}
    for name in greedy_ref.GOLDEN_CASES:
        cfg, sd, _, _, ml = greedy_ref.golden_inputs(name)
        m = mg.ref_t5(cfg, sd)
        for seed in range(1, limit):
            _, _, ids, mask, _ = greedy_ref.golden_inputs(name, seed)
            out, steps = _generate(m, torch.from_numpy(ids), torch.from_numpy(mask), cfg, ml)
            B, width = out.shape
            chosen, gap = np.zeros((width - 1, B), np.float32), np.zeros((width - 1, B), np.float32)
            smallest = np.inf
            for s, lg in enumerate(steps):
                top2 = torch.topk(lg, 2, dim=-1).values
                chosen[s], gap[s] = top2[:, 0].numpy(), (top2[:, 0] - top2[:, 1]).numpy()
                unfinished = ~(out[:, 1:s + 1] == cfg.eos_token_id).any(dim=1).numpy()   # rows that have not emitted EOS before step s
                smallest = min(smallest, float(gap[s][unfinished].min()))
            print(f"{name}: seed {seed}, width {width}, smallest deciding gap {smallest:.3e}", flush=True)
            if smallest >= greedy_ref.GAP:
                break
        else:
            raise SystemExit(f"{name}: no seed below {limit} clears {greedy_ref.GAP}")
        arrays.update({f"{name}_input_ids": ids.astype(np.int16), f"{name}_attention_mask": mask.astype(np.int8), f"{name}_ids": out,
                       f"{name}_chosen": chosen, f"{name}_gap": gap, f"{name}_token_seed": seed, f"{name}_min_gap": smallest,
                       f"{name}_max_length": ml})
    mg.save("g18_generate_greedy", seed=greedy_ref.SD_SEED, **arrays)


def pick_seeds(limit=200):
    for name, (_, lens, _, _, _, bf16) in greedy_ref.ORACLE_CASES.items():
        for seed in range(1, limit):
            _, _, trace = greedy_ref.run_oracle(name, seed)
            if bf16:
                share = float(greedy_ref.close_rows(trace, greedy_ref.BF16_GAP).float().mean())
                ok, what = share < 0.1, f"share of rows with a gap below {greedy_ref.BF16_GAP:g}: {share:.4f}"
            else:
                g = greedy_ref.min_gap(trace)
                ok, what = g >= greedy_ref.GAP, f"smallest deciding gap {g:.3e}"
            if ok:
                print(f"{name}: seed {seed} ({what})", flush=True)
                break
        else:
            print(f"{name}: no seed below {limit}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", action="store_true")
    a = ap.parse_args()
    pick_seeds() if a.seeds else g_generate_greedy()
