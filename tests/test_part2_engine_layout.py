"""Host side of the Part 2 shape engine (project-nerf_amd/part2.py), no GPU and no library: which shapes it accepts, the flat
parameter layout against NeuralField's own, and the float64 restatement of the decoder that tests/test_gpu_part2_engine.py uses as
its "matched" reference -- pinned here, with its rounding switched off, to the reference's own output and gradients (g16)."""
import os

import numpy as np
import pytest
import torch

from project_nerf_amd import part2
from project_nerf_amd.core import NeuralField

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g16_nerf_shapes.npz")


def make_cfg(H, layers, skip, V, L, Ld, **kw):
    cfg = {"mode": "part2_nerf", "use_positional_encoding": True, "L_embed": L, "use_viewdirs": True, "L_embed_dir": Ld,
           "hidden_dim": H, "num_layers": layers, "skip_layer": skip, "view_dim": V}
    cfg.update(kw)
    return cfg


# ---------------------------------------------------------------------------------------------- float64 restatement
def st_bf16(x):
    """bf16 rounding of a float64 tensor, straight-through for autograd"""
    return x + (x.detach().float().bfloat16().double() - x.detach())


def fourier_cpu(x, L):
    """reference src/embeddings.py:22-32 in fp32 on the CPU"""
    out = [x]
    for freq in 2.0 ** torch.linspace(0.0, L - 1, steps=L) if L > 0 else []:
        out += [torch.sin(x * freq * np.pi), torch.cos(x * freq * np.pi)]
    return torch.cat(out, dim=-1)


def decoder64(shape, W, x_enc, d_enc, rounded):
    """reference src/decoders.py:68-87 in float64 on the encoded inputs.  ``rounded``: the fused chain's rounding points -- bf16
    codes, bf16 weights, every hidden activation rounded after its relu, the feature vector rounded; biases and sums stay
    float64.  Returns rgb [n,3], sigma [n] and the hidden activations h_0..h_last, h_v (for relu-mask statistics)."""
    H, layers, skip, V, L, Ld = shape
    r = st_bf16 if rounded else (lambda t: t)
    w = lambda name: r(W[f"decoder.{name}.weight"])
    b = lambda name: W[f"decoder.{name}.bias"]
    x, d = r(x_enc.double()), r(d_enc.double())
    h, hs = x, []
    for i in range(layers):
        if i == skip:
            h = torch.cat([h, x], dim=-1)
        h = r(torch.relu(h @ w(f"pts_layers.{i}").T + b(f"pts_layers.{i}")))
        hs.append(h)
    sigma = torch.relu(h @ w("sigma_layer").T + b("sigma_layer"))[:, 0]
    feat = r(h @ w("feature_layer").T + b("feature_layer"))
    hv = r(torch.relu(torch.cat([feat, d], dim=-1) @ w("view_layer").T + b("view_layer")))
    hs.append(hv)
    return torch.sigmoid(hv @ w("rgb_layer").T + b("rgb_layer")), sigma, hs


def golden_case(tag):
    g = np.load(GOLDEN)
    shape = tuple(int(v) for v in g[f"{tag}:shape"])
    t = lambda k: torch.from_numpy(g[f"{tag}:{k}"])
    weights = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}:w:")}
    grads = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}:g:")}
    return dict(shape=shape, pts=t("pts"), dirs=t("dirs"), a=t("a"), b=t("b"), rgb=t("rgb"), sigma=t("sigma")[:, 0], weights=weights, grads=grads)


# ---------------------------------------------------------------------------------------------- supported()
CORNERS = [(64, 2, 1, 64, 1, 0), (256, 8, 7, 128, 10, 4), (128, 8, 8, 64, 10, 0), (64, 2, -1, 128, 1, 4), (256, 8, 4, 128, 10, 4),
           (128, 4, 2, 64, 10, 4), (64, 3, 99, 64, 5, 2)]


@pytest.mark.parametrize("shape", CORNERS)
def test_supported_accepts_the_corners_of_the_compiled_set(shape):
    assert part2.supported(make_cfg(*shape)) is None


@pytest.mark.parametrize("change,text", [
    (dict(hidden_dim=96), "hidden_dim=96 (compiled: 64, 128, 256)"), (dict(hidden_dim=512), "hidden_dim=512 (compiled: 64, 128, 256)"),
    (dict(num_layers=1), "num_layers=1 (compiled: 2..8)"), (dict(num_layers=9), "num_layers=9 (compiled: 2..8)"),
    (dict(skip_layer=0), "skip_layer=0 (compiled:"), (dict(view_dim=32), "view_dim=32 (compiled: 64, 128)"),
    (dict(L_embed=11), "L_embed=11 (compiled: 1..10)"), (dict(L_embed_dir=5), "L_embed_dir=5 (compiled: 0..4)"),
    (dict(use_positional_encoding=False), "use_positional_encoding=False (compiled:"), (dict(mode="part2_instant"), "mode=part2_instant (compiled: part2_nerf)"),
])
def test_supported_names_the_offending_key(change, text):
    cfg = make_cfg(128, 4, 2, 64, 10, 4, **change)
    why = part2.supported(cfg)
    assert why is not None and why.startswith(text), why
    with pytest.raises(NotImplementedError, match="not compiled for " + text.split(" ")[0]):
        part2.Part2Engine(cfg, device="cpu")          # refused before any library is loaded


# ---------------------------------------------------------------------------------------------- layout
LAYOUTS = [(64, 3, 1, 64, 4, 2), (128, 4, 4, 128, 10, 0), (128, 4, 2, 64, 10, 4), (256, 8, 4, 128, 10, 4), (64, 2, 1, 128, 1, 0)]


@pytest.mark.parametrize("shape", LAYOUTS)
def test_slice_table_is_the_modules_parameter_order(shape):
    cfg = make_cfg(*shape)
    model = NeuralField(cfg)
    named = [(k, tuple(p.shape)) for k, p in model.named_parameters()]
    table = part2.slice_table(cfg)
    assert [(k, s) for k, _, s in table] == named
    off = 0
    for _, o, s in table:                       # tiles [0, param_count)
        assert o == off
        off += int(np.prod(s))
    assert off == part2.param_count(cfg) == sum(p.numel() for p in model.parameters())


def test_flatten_unflatten_round_trip():
    cfg = make_cfg(64, 3, 1, 64, 4, 2)
    torch.manual_seed(3)
    model = NeuralField(cfg)
    flat = part2.flatten(cfg, model.state_dict())
    back = part2.unflatten(cfg, flat)
    assert flat.shape == (part2.param_count(cfg),)
    for k, p in model.named_parameters():
        assert torch.equal(back[k], p.detach())
    assert torch.equal(part2.flatten(cfg, back), flat)
    NeuralField(cfg).load_state_dict(back, strict=False)


def test_default_init_bounds():
    cfg = make_cfg(128, 4, 2, 64, 10, 4)
    flat = part2.default_init(cfg, seed=1)
    parts = part2.unflatten(cfg, flat)
    for k, v in parts.items():
        fan_in = parts[k.replace("bias", "weight")].shape[1]
        assert float(v.abs().max()) <= 1 / fan_in ** 0.5
        if v.numel() >= 64:
            assert float(v.abs().max()) > 0.9 / fan_in ** 0.5 and abs(float(v.mean())) < 0.2 / fan_in ** 0.5
    assert not torch.equal(flat, part2.default_init(cfg, seed=2)) and torch.equal(flat, part2.default_init(cfg, seed=1))


# ---------------------------------------------------------------------------------------------- the restatement vs g16
# fp32 against float64 on sums of at most 256 + 63 terms of magnitude <= a few: relative 6e-8 * sqrt(319) ~ 1e-6 per layer, six
# layers deep -> 1e-5 relative is ten times that; densities reach a few units, colours lie in (0, 1)
FP32_NOISE = 1e-5


@pytest.mark.parametrize("tag", ["a", "b"])
def test_unrounded_restatement_reproduces_the_reference(tag):
    c = golden_case(tag)
    H, layers, skip, V, L, Ld = c["shape"]
    W = {k: v.double().requires_grad_(True) for k, v in c["weights"].items()}
    assert list(W) == [k for k, _, _ in part2.slice_table(make_cfg(*c["shape"]))]
    rgb, sigma, _ = decoder64(c["shape"], W, fourier_cpu(c["pts"], L), fourier_cpu(c["dirs"], Ld), rounded=False)
    e_rgb = float((rgb.detach() - c["rgb"].double()).abs().max())
    e_sig = float(((sigma.detach() - c["sigma"].double()).abs() / c["sigma"].double().abs().clamp_min(1.0)).max())
    print(f"g16 {tag}: rgb max-abs {e_rgb:.3e}, sigma max-rel {e_sig:.3e}, zero densities {float((c['sigma'] == 0).float().mean()):.3f}")
    assert e_rgb <= FP32_NOISE and e_sig <= FP32_NOISE
    assert float((c["sigma"] == 0).float().mean()) < 0.5
    grads = torch.autograd.grad((rgb * c["a"].double()).sum() + (sigma * c["b"].double()[:, 0]).sum(), list(W.values()))
    for (k, _), g in zip(W.items(), grads):
        rel = float((g - c["grads"][k].double()).norm() / c["grads"][k].double().norm())
        print(f"  {k}: rel-L2 {rel:.3e}")
        assert rel <= FP32_NOISE, k
