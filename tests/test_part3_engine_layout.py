"""Host-side checks of the Part 3 engine (project-nerf_amd/part3.py): which configurations the fused chains accept, and
that the engine's flat-parameter slice table covers NeuralField('part3', canonical_type='instant') exactly."""
import math
import os

import pytest
import yaml

from conftest import ROOT


def example_cfg():
    return yaml.safe_load(open(os.path.join(ROOT, "configs", "part3_instant.yaml.example")))


def test_supported_accepts_the_example_config():
    from project_nerf_amd import part3
    cfg = example_cfg()
    assert cfg["engine"] is True and cfg["batch_size"] == 8192 and cfg["n_samples"] == 128
    assert part3.supported(cfg) is None
    # table size, base resolution, level scale and bound are free
    assert part3.supported(dict(cfg, log2_hashmap_size=14, base_resolution=8, per_level_scale=1.38, scene_bound=1.2)) is None


@pytest.mark.parametrize("key,value", [
    ("mode", "part4"), ("canonical_type", "nerf"), ("direct_time_conditioning", True), ("L_embed", 8), ("L_embed_time", 6),
    ("L_embed_dir", 2), ("deform_hidden_dim", 256), ("deform_num_layers", 6), ("hidden_dim", 128), ("n_levels", 12),
    ("n_features_per_level", 4),
])
def test_supported_names_the_rejected_key(key, value):
    from project_nerf_amd import part3
    why = part3.supported(dict(example_cfg(), **{key: value}))
    assert why is not None and key in why, why


def test_supported_rejects_a_missing_position_code():
    from project_nerf_amd import part3
    cfg = example_cfg()
    del cfg["L_embed"]                                   # NeuralField's default is 0: no Fourier code of x
    assert "L_embed" in part3.supported(cfg)


def test_slice_table_covers_the_module_state_dict_once():
    from project_nerf_amd import part3
    from project_nerf_amd.core import NeuralField
    cfg = dict(example_cfg(), log2_hashmap_size=12)
    model = NeuralField(cfg)
    params = dict(model.named_parameters())
    table = part3.Part3InstantEngine.slice_table()
    keys = [k for k, _, _, _ in table]
    assert sorted(keys) == sorted(params) and len(set(keys)) == len(keys)
    spans = []
    for key, region, off, shape in table:
        if region == "table":
            assert key == part3.TABLE_KEY
            continue
        assert tuple(params[key].shape) == tuple(shape), key
        spans.append((off, off + math.prod(shape)))
    spans.sort()
    for (a0, a1), (b0, _) in zip(spans, spans[1:]):
        assert a1 <= b0, "slices overlap"
    assert spans[-1][1] == part3.N_PARAMS
    # the canonical decoder sits at Part 4's offsets, the deformation MLP right behind the Part 4 vector
    from project_nerf_amd import part4
    assert dict((k, o) for k, _, o, _ in table)["decoder.sigma_net.params"] == part4.S1
    assert part3.DEFORM0 == part4.N_PARAMS
