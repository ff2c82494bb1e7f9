#!/usr/bin/env python3
"""Fixture for the checkpoint reader (tests/test_preprocess.py): the reference's r1/best-model-checkpoint.pt (written by
train-r1.py's save_ckp) -- DATA.  Kept as the reference wrote it (epoch, state_dict, optimizer, loss) except that the Adam
moment tensors (exp_avg, exp_avg_sq) are dropped from optimizer['state'] (2.4 MB -> 0.8 MB); each entry keeps its 'step'.

    python tests/golden/make_checkpoint_fixture.py <reference tree>   ->  tests/golden/checkpoint_r1_best.pt
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    ck = torch.load(os.path.join(ref, "r1", "best-model-checkpoint.pt"), map_location="cpu", weights_only=True)
    opt = ck["optimizer"]
    opt["state"] = {k: {"step": s["step"]} for k, s in opt["state"].items()}
    torch.save(ck, os.path.join(HERE, "checkpoint_r1_best.pt"))
    print("epoch", ck["epoch"], "loss", ck["loss"], "tensors", len(ck["state_dict"]))


if __name__ == "__main__":
    main(*sys.argv[1:])
