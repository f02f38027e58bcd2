"""nerf_p3_nerf_render_rays_fwd -- a frame of Part 3 with the 8x256 canonical field (standard and direct time conditioning) as one launch
chain whose field kernels read the frame's time from device memory -- against today's loop on the same inputs, built from existing ops:
per chunk ops.sample_rays(want_points=True) -> part3.deform_fwd with a torch.full time vector (skipped under direct time conditioning)
-> part3_nerf.canon_fwd -> ops.composite.  A sample's x_c and decoder outputs depend on its own point, direction and the time only, on
one MFMA column, and the scalar-time kernels run the same arithmetic on the same values, so every comparison is torch.equal on rgb,
depth and acc.  The fixture first checks on the LOOP that a comparison cannot pass vacuously: every ray accumulates something, the
time matters in both modes, and the deformation matters (W4 = b4 = 0 changes the standard frame).  Each test runs in about a second."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

from conftest import ROOT
from test_gpu_instant_render_chain import assert_same, crossing_rays
from test_gpu_part3_engine import deform_params
from test_gpu_part3_grid_update import _dynamic_scene
from test_gpu_part3_nerf_engine import MODES, cfg_of

pytestmark = pytest.mark.gpu

L8 = torch.linspace(0, 1, 8).tolist() # entries with no short binary form
W4 = 43904                            # csrc/p3deform.hip's flat layout: the output layer [3,128] and its bias end the vector


def make_engine(mode, seed=1, **over):
    """an engine whose field varies visibly over space and time: decoder weights 2.5 times their initial draw (the activations keep
    their size through the eight layers), a density bias above zero, and in standard mode a seeded deformation MLP whose output layer
    has standard deviation 0.05"""
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.part3_nerf import Part3NerfEngine
    cfg = cfg_of(mode, **over)
    torch.manual_seed(seed)
    model = NeuralField(cfg).cuda()
    with torch.no_grad():
        dec = model.decoder_direct if mode == "dtc" else model.decoder
        for name, p in dec.named_parameters():
            if name.endswith("weight"):
                p.mul_(2.5)
        dec.sigma_layer.bias.fill_(0.5)
        if mode == "standard":
            model.deform_net.load_state_dict(deform_params(seed + 2).state_dict())
    eng = Part3NerfEngine(cfg, seed=seed)
    eng.load_from_model(model)
    return eng


class Field:
    """what the entry reads, taken from an engine: both packed images (None for the deformation under direct time conditioning; in
    standard mode also the deformation image with W4 = b4 = 0)"""

    def __init__(self, eng):
        from project_nerf_amd import part3
        self.dtc = eng.dtc
        self.packed_c = eng.packed_c.clone()
        self.packed_d = None if eng.dtc else eng.packed_d.clone()
        self.packed_still = None
        if not eng.dtc:
            still = eng.deform_params.clone()
            assert float(still[W4:].abs().max()) > 0.0
            still[W4:] = 0
            self.packed_still = part3.deform_pack(still)
        self.bg = torch.ones(3, device="cuda")

    def loop(self, o, d, S, chunk, t, near=2.0, far=6.0, bg=None, packed_d=None, no_bg=False):
        """today's path chunk by chunk, from existing ops (a time vector per chunk, fresh tensors per step)"""
        from project_nerf_amd import ops, part3, part3_nerf
        bg = self.bg if bg is None else bg
        packed_d = self.packed_d if packed_d is None else packed_d
        outs = []
        with torch.no_grad():
            for i in range(0, o.shape[0], chunk):
                oc, dc = o[i:i + chunk].contiguous(), d[i:i + chunk].contiguous()
                r = oc.shape[0]
                b = None if no_bg else (bg[i:i + chunk].contiguous() if bg.dim() == 2 else bg)
                z, pts, dirs = ops.sample_rays(oc, dc, near, far, S, want_points=True)
                tv = torch.full((r * S,), float(t), device="cuda")
                x = pts if self.dtc else part3.deform_fwd(packed_d, pts, tv)[1]
                rgb, sigma = part3_nerf.canon_fwd(self.packed_c, x, tv, dirs)
                outs.append(ops.composite(rgb.view(r, S, 3), sigma.view(r, S), z, dc, b)[:3])
        return tuple(torch.cat([x[k] for x in outs], 0) for k in range(3))

    def chain(self, o, d, S, chunk, t, near=2.0, far=6.0, bg=None, workspace=None):
        from project_nerf_amd import ops
        return ops.p3_nerf_render_rays_fwd(self.packed_d, self.packed_c, o, d, S, near, far, torch.tensor([float(t)], device="cuda"),
                                           self.bg if bg is None else bg, chunk, workspace=workspace)


def checked_field(mode, **over):
    """a Field whose LOOP frame cannot make a comparison vacuous"""
    f = Field(make_engine(mode, **over))
    o, d = crossing_rays(40, seed=5)
    a = f.loop(o, d, 64, 40, 0.25)
    assert float(a[2].min()) > 0.0, "a ray accumulated nothing"
    later = f.loop(o, d, 64, 40, 0.75)
    assert not torch.equal(a[0], later[0]), "t = 0.25 and t = 0.75 give the same frame: the time does not matter"
    changed = -1
    if mode == "standard":
        still = f.loop(o, d, 64, 40, 0.25, packed_d=f.packed_still)
        assert not torch.equal(a[0], still[0]), "W4 = b4 = 0 leaves the frame unchanged: the deformation does not matter"
        changed = int((a[0] != still[0]).sum())
    print(f"[p3 nerf loop {mode} {over}] acc {float(a[2].min()):.3g} .. {float(a[2].max()):.3g}; rgb std {float(a[0].std()):.3g}; "
          f"{changed} values change with W4 = b4 = 0, {int((a[0] != later[0]).sum())} between t = 0.25 and 0.75")
    return f


@pytest.fixture(scope="module")
def fields():
    import project_nerf_amd  # noqa: F401
    return {mode: checked_field(mode) for mode in MODES}


def workspace(chunk, S, fill=None):
    from project_nerf_amd import ops
    ws = torch.empty(ops.p3_nerf_render_workspace_bytes(chunk, S), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


# ------------------------------------------------------------------ 2. tile edges
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R,S", [(1, 2), (1, 255), (3, 85), (1, 256), (2, 128), (1, 257), (5, 77), (2, 500), (1, 1024)])
def test_tile_edges(fields, mode, R, S):
    """row counts 2, 255, 255, 256, 256, 257, 385, 1000 and 1024: below, at and just above one 256-row tile of both chains, more than
    one tile, and the largest sample count"""
    f = fields[mode]
    o, d = crossing_rays(R, seed=R * 2000 + S)
    assert_same(f.chain(o, d, S, R, L8[3]), f.loop(o, d, S, R, L8[3]), f"{mode} {R} x {S}")


# ------------------------------------------------------------------ 3. chunking and backgrounds
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bg", ["none", "one", "per_ray"])
def test_ragged_last_chunk_and_backgrounds(fields, mode, bg):
    """7 rays at chunk 3: chunks of 3, 3 and 1 ray"""
    f = fields[mode]
    o, d = crossing_rays(7, seed=31)
    g = torch.Generator().manual_seed(32)
    b = {"none": None, "one": torch.rand(3, generator=g).cuda(), "per_ray": torch.rand(7, 3, generator=g).cuda()}[bg]
    if b is None:
        from project_nerf_amd import ops
        got = ops.p3_nerf_render_rays_fwd(f.packed_d, f.packed_c, o, d, 48, 2.0, 6.0, torch.tensor([L8[2]], device="cuda"), None, 3)
        want = f.loop(o, d, 48, 3, L8[2], no_bg=True)
    else:
        got, want = f.chain(o, d, 48, 3, L8[2], bg=b), f.loop(o, d, 48, 3, L8[2], bg=b)
    assert_same(got, want, f"{mode} bg {bg}")


@pytest.mark.parametrize("mode", MODES)
def test_a_chunk_larger_than_the_ray_count(fields, mode):
    f = fields[mode]
    o, d = crossing_rays(7, seed=33)
    assert_same(f.chain(o, d, 48, 1000, L8[5]), f.loop(o, d, 48, 7, L8[5]), mode)


# ------------------------------------------------------------------ 4. workspace
@pytest.mark.parametrize("mode", MODES)
def test_workspace_contents_never_matter(fields, mode):
    f = fields[mode]
    o, d = crossing_rays(11, seed=41)
    a = f.chain(o, d, 40, 4, L8[1], workspace=workspace(4, 40, 0xFF))
    b = f.chain(o, d, 40, 4, L8[1], workspace=workspace(4, 40, 0))
    assert_same(a, b, "0xFF-filled against zeroed")
    assert_same(a, f.loop(o, d, 40, 4, L8[1]), "against the loop")


@pytest.mark.parametrize("mode", MODES)
def test_a_small_call_after_a_large_one_on_one_buffer(fields, mode):
    f = fields[mode]
    ws = workspace(40, 128)
    o, d = crossing_rays(40, seed=43)
    assert_same(f.chain(o, d, 128, 40, L8[4], workspace=ws), f.loop(o, d, 128, 40, L8[4]), "40 x 128")
    o, d = crossing_rays(1, seed=44)
    assert_same(f.chain(o, d, 127, 1, L8[6], workspace=ws), f.loop(o, d, 127, 1, L8[6]), "1 x 127 on the same buffer")


@pytest.mark.parametrize("mode", MODES)
def test_nothing_is_written_behind_the_workspace(fields, mode):
    """a workspace of exactly workspace_bytes, an 8 KiB guard band behind it"""
    from project_nerf_amd import ops
    f = fields[mode]
    R, S = 5, 77
    need = ops.p3_nerf_render_workspace_bytes(R, S)
    buf = torch.full((need + 8192,), 0xA5, dtype=torch.uint8, device="cuda")
    o, d = crossing_rays(R, seed=45)
    got = f.chain(o, d, S, R, L8[2], workspace=buf[:need])
    torch.cuda.synchronize()
    assert bool((buf[need:] == 0xA5).all()), "the guard band was written"
    assert bool((buf[:need] != 0xA5).any())
    assert_same(got, f.loop(o, d, S, R, L8[2]), mode)


# ------------------------------------------------------------------ 5. time word
@pytest.mark.parametrize("mode", MODES)
def test_the_time_word_is_read_from_the_device(fields, mode):
    from project_nerf_amd import ops
    f = fields[mode]
    o, d = crossing_rays(9, seed=51)
    word, ws = torch.tensor([L8[1]], device="cuda"), workspace(4, 64)

    def call():
        return ops.p3_nerf_render_rays_fwd(f.packed_d, f.packed_c, o, d, 64, 2.0, 6.0, word, f.bg, 4, workspace=ws)

    first = call()
    assert_same(first, f.loop(o, d, 64, 4, L8[1]), "first time")
    word.fill_(L8[6])
    second = call()
    assert_same(second, f.loop(o, d, 64, 4, L8[6]), "after the word was overwritten in place")
    assert not torch.equal(first[0], second[0])


@pytest.mark.parametrize("L", [0, 3, 10])
def test_direct_time_conditioning_at_other_time_code_widths(L):
    f = checked_field("dtc", L_embed_time=L)        # L 0: the time code is the time itself, and it still matters
    o, d = crossing_rays(9, seed=53)
    for t in (0.25, L8[5]):
        assert_same(f.chain(o, d, 64, 4, t), f.loop(o, d, 64, 4, t), f"L_embed_time {L}, t = {t}")


# ------------------------------------------------------------------ 6. graph
@pytest.mark.parametrize("mode", MODES)
def test_graph_capture(fields, mode):
    """A capture that completes shows the entry neither allocates nor synchronises; a replay after the rays, both packed images, the
    background AND the time word were overwritten IN PLACE renders the new field at the new time (the graph holds pointers, not
    values).  The chain is linear, on one stream (the process keeps its default number of hardware queues)."""
    from project_nerf_amd import ops
    f = fields[mode]
    other = Field(make_engine(mode, seed=2))
    R, S, chunk = 12, 64, 5
    o, d = [t.clone() for t in crossing_rays(R, seed=61)]
    bg = f.bg.clone()
    packed_c = f.packed_c.clone()
    packed_d = None if f.dtc else f.packed_d.clone()
    time = torch.tensor([0.25], device="cuda")
    ws = workspace(chunk, S)

    def call():
        return ops.p3_nerf_render_rays_fwd(packed_d, packed_c, o, d, S, 2.0, 6.0, time, bg, chunk, workspace=ws)

    eager = [t.clone() for t in call()]
    assert_same(eager, f.loop(o, d, S, chunk, 0.25), "eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, eager, "first replay")
    o2, d2 = crossing_rays(R, seed=62)
    o.copy_(o2)
    d.copy_(d2)
    packed_c.copy_(other.packed_c)
    if not f.dtc:
        packed_d.copy_(other.packed_d)
    bg.copy_(torch.tensor([0.25, 0.5, 0.75]))
    time.fill_(L8[5])
    g.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    assert_same(replayed, other.loop(o, d, S, chunk, L8[5], bg=bg), "replay against the loop on the new values")
    assert not torch.equal(replayed[0], eager[0])
    # the time word alone: a replay at another time differs from the one before it and equals the loop at that time
    time.fill_(L8[2])
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out[0], replayed[0])
    assert_same(out, other.loop(o, d, S, chunk, L8[2], bg=bg), "replay at another time")


# ------------------------------------------------------------------ 7. engine
@pytest.mark.parametrize("mode", MODES)
def test_engine_method(mode):
    """render_image_chain == render_image(chain=False) on a trained-a-little engine"""
    from project_nerf_amd import ops
    eng = make_engine(mode, seed=3)
    o, d = crossing_rays(256, seed=71)
    gen = torch.Generator().manual_seed(72)
    target, t = torch.rand(256, 3, generator=gen).cuda(), torch.rand(256, 1, generator=gen).cuda()
    for _ in range(3):
        eng.train_step(o, d, target, t, 32)
    vo, vd = crossing_rays(24 * 24, seed=73)
    vo, vd = vo.view(24, 24, 3), vd.view(24, 24, 3)
    bg = torch.tensor([0.25, 0.5, 0.75], device="cuda")
    S = 32
    for time, kw in ((torch.tensor(L8[3]), {}), (torch.tensor([[L8[6]]]).cuda(), dict(bg=bg))):
        a = eng.render_image_chain(vo, vd, time, S, chunk=100, **kw)
        b = eng.render_image(vo, vd, time, S, chunk=100, chain=False, **kw)
        assert a.shape == b.shape == (24, 24, 3)
        assert torch.equal(a, b), f"{int((a != b).sum())} values differ"
        assert float((b - (eng.bg if not kw else bg)).abs().max()) > 0.0           # not a frame of background
    assert list(eng._chain_ws) == [(100, S)]             # the workspace is kept per (chunk, n_samples)
    ws, word = eng._chain_ws[(100, S)], eng._chain_time
    n = 100 * S
    per_piece = sum((n * b + 255) // 256 * 256 for b in (4, 12, 12, 12, 4, 12))
    assert ws.numel() == per_piece == 100 * S * 56 == ops.p3_nerf_render_workspace_bytes(100, S)
    assert float(word) == torch.tensor(L8[6]).item()
    eng.render_image_chain(vo, vd, torch.tensor(0.5), S, chunk=100)
    assert eng._chain_ws[(100, S)] is ws and eng._chain_time is word and float(word) == 0.5          # both persistent
    eng.render_image_chain(vo, vd, torch.tensor(0.5), 16, chunk=100)
    assert set(eng._chain_ws) == {(100, S), (100, 16)}
    with pytest.raises(NotImplementedError, match="Part3NerfEngine"):        # the keyword stays refused: the chain is a method of its own
        eng.render_image(vo, vd, torch.tensor(0.5), 16, chain=True)


# ------------------------------------------------------------------ 8. YAML
def test_run_py_renders_through_the_chain(tmp_path):
    root = _dynamic_scene(str(tmp_path / "dyn"))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part3_dtc.yaml.example")))
    cfg.update(train_iters=24, batch_size=512, log_every=8, val_every=24, downscale=1, n_samples=32, render_n_samples=32, grid_warmup_iters=8,
               random_bg_start=16, log_dir=str(tmp_path / "out"), engine=True, render_chain=True)
    cfg_path = tmp_path / "part3_dtc.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "--config", str(cfg_path), "--data_dir", root, "--render_n", "1"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "render_chain" in r.stdout and "nerf_p3_nerf_render_rays_fwd" in r.stdout, r.stdout[-2000:]
    assert "[Validation] PSNR" in r.stdout and "Test PSNR" in r.stdout, r.stdout[-2000:]
