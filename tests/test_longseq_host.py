"""The CPU oracle of the doc tower against the reference's own DPRContextEncoder at 512 tokens (tests/golden/g16_doc_tower_long.npz,
made by tests/golden/make_golden_longseq.py): pins the oracle that tests/test_gpu_longseq.py leans on above 128 tokens."""
import numpy as np
import torch

from conftest import golden
from gdr_amd import synth
from oracle import bert_ref

torch.set_grad_enabled(False)

CASES = {"tiny": lambda: dict(synth.bert_config(True), max_pos=512), "base": lambda: synth.bert_config(False)}


def test_oracle_doc_tower_matches_reference_at_512_tokens():
    g = golden("g16_doc_tower_long")
    for name, make in CASES.items():
        bc = make()
        sd = synth.make_bert_state_dict(bc, seed=int(g["seed"]))
        ids, mask = torch.from_numpy(g[name + "_ids"].astype(np.int64)), torch.from_numpy(g[name + "_mask"].astype(np.int64))
        assert ids.shape[1] == 512 and int(mask[0].sum()) == 512
        hid, pooled = bert_ref.bert_forward(sd, bc, ids, mask)
        rows = g[name + "_rows"]
        live = (mask[:, rows] != 0).numpy()
        dp = float(np.abs(pooled.numpy() - g[name + "_pooled"]).max())
        dh = float(np.abs(hid[:, rows].numpy() - g[name + "_hidden"])[live].max())
        print(f"g16 {name}: oracle vs reference max |pooled| {dp:.2e}, |hidden (live rows)| {dh:.2e}")
        assert dp <= 1e-5 and dh <= 1e-5
