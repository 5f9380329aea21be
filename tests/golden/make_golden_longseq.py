#!/usr/bin/env python3
"""Generate tests/golden/g16_doc_tower_long.npz: the REFERENCE's doc tower `DPRContextEncoder(DPRConfig(...))` (modeling_dpr.py:146-191
over modeling_bert.py) at the passage length its corpus embedder runs at (Data_process/NQ_dataset/bert/bert_NQ.sh:5 MAX_LEN=512), on CPU
through make_golden's import shims.

Build-container only, like make_golden.py: only the arrays written here (inputs + the reference's outputs) are committed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_longseq.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import make_golden            # noqa: E402
from gdr_amd import synth     # noqa: E402

SEED_W, SEED_T, L = 4321, 17, 512
CASES = (  # name, config, B, min_len, sampled rows of the last hidden state
    ("tiny", dict(synth.bert_config(True), max_pos=512), 6, 100, [0, 1, 127, 128, 129, 255, 256, 300, 511]),
    ("base", synth.bert_config(False), 2, 200, [1, 64, 127, 128, 300, 511]),
)


def main():
    with contextlib.redirect_stdout(io.StringIO()):
        make_golden.import_reference()
    from transformers.configuration_dpr import DPRConfig
    from transformers.modeling_dpr import DPRContextEncoder
    out = {}
    for name, bc, B, min_len, rows in CASES:
        cfg = DPRConfig(vocab_size=bc["vocab_size"], hidden_size=bc["hidden_size"], num_hidden_layers=bc["num_layers"],
                        num_attention_heads=bc["num_heads"], intermediate_size=bc["d_ff"],
                        max_position_embeddings=bc["max_pos"], type_vocab_size=bc["type_vocab"], projection_dim=0)
        m = DPRContextEncoder(cfg)
        sd = synth.make_bert_state_dict(bc, seed=SEED_W)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        assert not unexpected and all(("pooler" in k or "position_ids" in k) for k in missing), (missing, unexpected)
        m.eval()
        ids, mask = synth.make_tokens(B, L=L, vocab_hi=bc["vocab_size"], seed=SEED_T, min_len=min_len)
        mask[0, :] = 1                                   # one full-length passage (its ids past the drawn length stay PAD ids)
        with torch.no_grad():
            o = m(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), return_dict=True, output_hidden_states=True)
        out[name + "_ids"], out[name + "_mask"] = ids.astype(np.int32), mask.astype(np.int8)
        out[name + "_pooled"] = o.pooler_output.numpy()
        out[name + "_rows"] = np.array(rows, np.int64)
        out[name + "_hidden"] = o.hidden_states[-1][:, rows].numpy()
        print(name, "lengths", mask.sum(1).tolist())
    path = os.path.join(HERE, "g16_doc_tower_long.npz")
    np.savez_compressed(path, seed=np.int64(SEED_W), **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
