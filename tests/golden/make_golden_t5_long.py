#!/usr/bin/env python3
"""Generate tests/golden/g17_t5_long.npz by running the REFERENCE's T5Stack and generate() above 128 input tokens (build container
only, like make_golden.py, whose import shims and helpers it uses): the t64 config of tests/t5_long.py with this repo's seeded
synthetic weights.  Arrays only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_t5_long.py            # writes g17_t5_long.npz
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_t5_long.py --seeds    # prints the token seeds of tests/t5_long.GEN_CASES

--seeds needs no reference: for every generate() case it runs the CPU oracle with token seeds 1, 2, ... and prints the first one
whose search clears t5_long.GAP at every cut and between adjacent final scores (t5_long.margins).
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
import t5_long                # noqa: E402


def g_t5_long():
    mg.import_reference()
    cfg = t5_long.t64()
    sd = t5_long.state_dict("t64")
    m = mg.ref_t5(cfg, sd)
    # encoder: B = 3, L = 300, lengths 300 / 131 / 17
    ids, mask = t5_long.tokens_with_lengths((300, 131, 17), 300, cfg.vocab_size, seed=17)
    with torch.no_grad():
        h = m.get_encoder()(torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), return_dict=True).last_hidden_state
    live = mask != 0
    # generate(): B = 2, L = 200, 4 beams
    gids, gmask = t5_long.tokens_with_lengths((200, 140), 200, cfg.vocab_size, seed=18)
    outs, scores, enc, steps = mg._generate(m, torch.from_numpy(gids), torch.from_numpy(gmask), cfg, R=4)
    mg.save("g17_t5_long", enc_ids=ids.astype(np.int16), enc_mask=mask.astype(np.int8), enc_hidden_live=h.numpy()[live],
            gen_ids=gids.astype(np.int16), gen_mask=gmask.astype(np.int8), gen_decoded=outs, gen_scores=np.array(scores, np.float64),
            gen_step_scores=torch.stack([s for s, _ in steps]), gen_step_tokens=torch.stack([t for _, t in steps]),
            num_beams=4, length_penalty=0.8, seed=t5_long.SD_SEED)


def pick_seeds(limit=200):
    for name, (kind, R, L, lens, ml, _, _) in t5_long.GEN_CASES.items():
        cfg = t5_long.CONFIGS[kind]()
        for seed in range(1, limit):
            rd, rs, trace, _, _ = t5_long.run_oracle(name, seed)
            step, fin = t5_long.margins(trace, rs, len(lens), R, cfg.decode_vocab_size)
            if step > t5_long.GAP and fin > t5_long.GAP:
                print(f"{name}: seed {seed} (cut gap {step:.2e}, final gap {fin:.2e})", flush=True)
                break
        else:
            print(f"{name}: no seed below {limit}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", action="store_true")
    a = ap.parse_args()
    pick_seeds() if a.seeds else g_t5_long()
