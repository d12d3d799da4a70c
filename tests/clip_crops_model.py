"""A stand-in for the CLIP image encoder in the crop tests and fixtures: ``encode_image`` gathers D
fixed positions of every [3, S, S] input, so its output is exact data movement and any difference
in the crops shows in the features."""
from __future__ import annotations

import numpy as np

D = 16


def gather_positions(out_size=224, dim=D, seed=7):
    return np.sort(np.random.default_rng(seed).choice(3 * out_size * out_size, dim, replace=False)).astype(np.int64)


class GatherModel:
    def __init__(self, positions):
        self.positions = np.asarray(positions, np.int64)

    def cuda(self):
        return self

    def eval(self):
        return self

    def encode_image(self, x):
        import torch
        pos = torch.as_tensor(self.positions, device=x.device)
        return x.reshape(x.shape[0], -1)[:, pos]
