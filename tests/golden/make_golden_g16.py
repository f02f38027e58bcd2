"""g16: the REFERENCE's NeuralField('part2_nerf') at two small decoder shapes (build container only, CPU).

Imports the read-only reference the way make_golden.py does and stores data only: the weights, 300 fixed points / view
directions, rgb, sigma, two random cotangents a, b and the autograd gradient of sum(rgb * a) + sum(sigma * b) with respect to every
parameter.  The sigma head's bias is drawn positive so that fewer than half of the stored densities are zero (checked here).

    python tests/golden/make_golden_g16.py      ->  tests/golden/g16_nerf_shapes.npz
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
# only the reference may provide `src` (make_golden.py)
sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) not in (ROOT, HERE)]
sys.path.insert(0, REF)
os.chdir(REF)

from src.core import NeuralField  # noqa: E402

# tag: (hidden_dim, num_layers, skip_layer, view_dim, L_embed, L_embed_dir); skip_layer == num_layers: no skip
SHAPES = {"a": (64, 3, 1, 64, 4, 2), "b": (128, 4, 4, 128, 10, 0)}
N = 300


def config(shape):
    H, layers, skip, V, L, Ld = shape
    return {"mode": "part2_nerf", "use_positional_encoding": True, "L_embed": L, "use_viewdirs": True, "L_embed_dir": Ld,
            "hidden_dim": H, "num_layers": layers, "skip_layer": skip, "view_dim": V}


def main():
    import src.core as probe
    assert probe.__file__.startswith(REF), probe.__file__
    out = {}
    for seed, (tag, shape) in enumerate(SHAPES.items()):
        torch.manual_seed(160 + seed)
        model = NeuralField(config(shape))
        g = torch.Generator().manual_seed(1600 + seed)
        with torch.no_grad():
            model.decoder.sigma_layer.bias.copy_(torch.rand(1, generator=g) * 0.04)
        pts = (torch.rand(N, 3, generator=g) * 2 - 1) * 1.5
        dirs = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
        a, b = torch.randn(N, 3, generator=g), torch.randn(N, 1, generator=g)
        rgb, sigma = model(pts, dirs)
        dead = float((sigma == 0).float().mean())
        assert dead < 0.5, f"shape {tag}: {dead:.2f} of the densities are zero"
        params = dict(model.named_parameters())
        grads = torch.autograd.grad((rgb * a).sum() + (sigma * b).sum(), list(params.values()))
        out[f"{tag}:shape"] = np.asarray(shape, dtype=np.int32)
        for k, v in (("pts", pts), ("dirs", dirs), ("a", a), ("b", b), ("rgb", rgb), ("sigma", sigma)):
            out[f"{tag}:{k}"] = v.detach().numpy().astype(np.float32)
        for (k, p), gr in zip(params.items(), grads):
            out[f"{tag}:w:{k}"] = p.detach().numpy().astype(np.float32)
            out[f"{tag}:g:{k}"] = gr.numpy().astype(np.float32)
        print(f"shape {tag} {shape}: {sum(p.numel() for p in params.values())} parameters, zero densities {dead:.3f}")
    path = os.path.join(HERE, "g16_nerf_shapes.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
