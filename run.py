#!/usr/bin/env python
"""Entry point with the reference's command line (run.py:2334-2376):

    python run.py --config configs/part2.yaml --data_dir data/nerf_synthetic/lego
                  [--checkpoint x.pth] [--eval_only] [--render_n N] [--render_chunk C]

Only the static hot path is built (modes part2_nerf, part2_instant); the loops below are this
repository's own counterparts of run_part2 / run_part2_instant and drive the MI355X kernels
through the reference's module surface (NeuralField, render_rays, DensityGrid, BlenderDataset).
Checkpoints use the reference format: {"model_state_dict", "config"[, "step", "val_psnr", "density_grid"]}.

Data parallelism (the reference is single-process): launched as
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 run.py --config ...
every rank holds a replica, forms ITS shard of one global batch (``batch_size`` stays the global batch), the flat
gradients are summed over RCCL/xGMI (overlapped with the backward pass) and averaged, gradient clipping happens after
the all-reduce, optimiser steps are replicated; evaluation renders row bands and gathers them on rank 0, which alone
prints, logs and writes checkpoints.  The process group is created before the first GPU call.
"""
import argparse
import os

import numpy as np
import torch
import yaml

from src.core import NeuralField
from src.dataset import BlenderDataset
from src.renderer import DensityGrid, render_image, render_rays, render_rays_nerf_grid_chain
from src.utils import TensorBoardLogger, compute_psnr, compute_psnr_torch, render_image_safe


GRID_FUSED_BATCH = True      # train_density_grid: the grid step's batch from nerf_train_batch_compact


def _target(rgba, bg):
    rgb, a = rgba[:, :3], rgba[:, 3:4]
    return rgb * a + bg * (1.0 - a)


def run_part2(cfg, args):
    """Vanilla NeRF training / evaluation (reference run.py:240-393)."""
    if not args.data_dir:
        raise ValueError("Part 2 requires --data_dir pointing to a NeRF dataset root.")
    if not torch.cuda.is_available():
        raise RuntimeError("the NeRF hot path runs on a HIP device only (no CPU fallback)")
    from project_nerf_amd import parallel
    rank, world = parallel.rank_world()
    main_rank = rank == 0
    say = print if main_rank else (lambda *a, **k: None)
    device = torch.device("cuda", torch.cuda.current_device())
    downscale, white_bkgd = cfg.get("downscale", 1), cfg.get("white_bkgd", True)
    scene_scale = cfg.get("scene_scale", 1.0)
    near, far = float(cfg.get("near", 2.0)), float(cfg.get("far", 6.0))
    n_samples = cfg.get("n_samples", 64)
    render_n_samples = cfg.get("render_n_samples", n_samples)
    batch_size, train_iters = cfg.get("batch_size", 4096), cfg.get("train_iters", 20000)
    lr, log_every, save_every = cfg.get("learning_rate", 5e-4), cfg.get("log_every", 100), cfg.get("save_every", 2000)
    chunk = args.render_chunk or cfg.get("chunk", 8192)
    log_dir = cfg.get("log_dir", "output/part2")
    ckpt_dir, render_dir = os.path.join(log_dir, "checkpoints"), os.path.join(log_dir, "renders")
    os.makedirs(ckpt_dir, exist_ok=True)
    os.makedirs(render_dir, exist_ok=True)

    train_set = BlenderDataset(args.data_dir, "train", downscale, white_bkgd, scene_scale).to(device)   # frames resident in HBM
    test_split = "test" if os.path.exists(os.path.join(args.data_dir, "transforms_test.json")) else "val"
    test_set = BlenderDataset(args.data_dir, test_split, downscale, white_bkgd, scene_scale)

    model = NeuralField(cfg).to(device)
    # use_density_grid: true (default false for this mode) -- an occupancy grid of the trained field, saved with the checkpoints in
    # the reference's format; evaluation then pushes only the active samples through the decoder (render_rays_nerf_grid_chain)
    grid, grid_loaded = None, False
    if cfg.get("use_density_grid", False):
        if not getattr(model.decoder, "fused", False):
            raise ValueError("use_density_grid: true needs the default decoder shape (hidden 256, 8 layers, skip 4, view 128)")
        grid = DensityGrid(cfg.get("grid_resolution", 128), cfg.get("scene_bound", 1.5), cfg.get("grid_threshold", 0.01)).to(device)
    # train_density_grid: true (default false) -- after grid_warmup_iters dense steps the training steps go through the grid too:
    # only the active samples reach the decoder's forward and backward (VanillaNerfEngine's grid step)
    train_grid = bool(cfg.get("train_density_grid", False)) and not args.eval_only
    if train_grid and grid is None:
        raise ValueError("train_density_grid: true needs use_density_grid: true (the steps go through the grid that is saved with the "
                         "checkpoints and used for evaluation)")
    if args.checkpoint:
        ckpt = torch.load(args.checkpoint, map_location=device)
        model.load_state_dict(ckpt["model_state_dict"])
        say(f">>> Loaded checkpoint: {args.checkpoint}")
        if grid is not None and "density_grid" in ckpt:
            grid.load_state_dict(ckpt["density_grid"])
            grid_loaded = True
            say(f">>> Density grid: loaded from the checkpoint ({float(grid.binary_grid.float().mean()) * 100:.1f} % of the cells occupied)")
        del ckpt

    def refresh_grid():
        """the grid of the model's current weights (DensityGrid.update, reference src/renderer.py:35-132)"""
        ratio = grid.update(model, device=device)
        say(f">>> Density grid: rebuilt from the model ({ratio * 100:.1f} % of the cells occupied)")

    def save_checkpoint(path):
        """reference format; with a grid: refreshed from the weights being saved and stored under "density_grid" """
        out = {"model_state_dict": model.state_dict(), "config": cfg}
        if grid is not None:
            refresh_grid()
            out["density_grid"] = grid.state_dict()
        torch.save(out, path)
    local_batch = parallel.check_global_batch(batch_size, world)   # this rank's shard of the global batch
    parallel.broadcast_([p.data for p in model.parameters()])       # replicas start from rank 0's weights whatever the seeds did
    first_ray = rank * local_batch
    if world > 1:
        say(f">>> data parallel: {world} ranks x {local_batch} rays (global batch {local_batch * world}), RCCL all-reduce of the flat gradient")

    # The reference's default decoder shape trains on the flat-parameter engine (what bench.py times: one kernel for the
    # batch draw, fused compositing + loss + backward, fused Adam + weight repack); its weights are copied into the
    # NeuralField for checkpoints and evaluation.  Other shapes, or `engine: false` in the YAML, take the module path
    # (NeuralField + render_rays + torch.optim.Adam, about twice the step time).
    dec = model.decoder
    use_engine = (not args.eval_only and cfg.get("engine", True) and getattr(dec, "fused", False)
                  and (dec.pos_dim, dec.dir_dim) == (63, 27))
    # A non-default shape trains on the fused chain of project-nerf_amd/part2.py only when the YAML says `engine: true`
    # explicitly (single rank, a shape the chain is compiled for); with the key absent it takes the module path.
    p2_eng = None
    if not use_engine and not args.eval_only and cfg.get("engine") is True:
        from project_nerf_amd import part2
        why = f"world size {world} (the engine is single-rank)" if world > 1 else part2.supported(cfg)
        if why is None:
            p2_eng = part2.Part2Engine(cfg, device=str(device), lr=lr, near=near, far=far, white_bkgd=white_bkgd)
            p2_eng.load_from_model(model)
            say(f">>> Part 2 on the fused HIP shape engine ({p2_eng.params.numel()} parameters)")
        else:
            say(f">>> Part 2 engine not used: {why}; training on the module path")
    if train_grid and p2_eng is not None:
        raise ValueError("train_density_grid: true: the shape engine (engine: true at a non-default decoder shape) has no grid step; "
                         "only the default-shape engine trains through the grid")
    if train_grid and not use_engine:
        raise ValueError("train_density_grid: true: the module path (engine: false, or a non-default decoder shape) has no grid step; "
                         "only the default-shape engine trains through the grid")
    if use_engine and train_grid:
        from project_nerf_amd.engine import VanillaNerfEngine
        from project_nerf_amd.flat_engine import grid_refresh_due
        tb = TensorBoardLogger(os.path.join(log_dir, "tensorboard")) if main_rank else None
        seed = int(cfg.get("seed", 0) or 0)
        eng = VanillaNerfEngine(params=dec.flat_parameters(), device=str(device), lr=lr, near=near, far=far, white_bkgd=white_bkgd,
                                seed=seed, world_size=world, grid_resolution=grid.resolution, bound=grid.bound,
                                grid_threshold=grid.threshold)
        sync_async = parallel.allreduce_sum_async if world > 1 else None
        warm, stop = cfg.get("grid_warmup_iters", 256), cfg.get("grid_stop_ratio", 0.9)
        # the batch of a grid step from ONE kernel (train_batch_compact) or from two (train_batch + prepare_batch): DESIGN.md 4.21
        # has both timings; `grid_fused_batch:` overrides the default
        fused_batch = bool(cfg.get("grid_fused_batch", GRID_FUSED_BATCH))

        def sync_model():
            model.load_state_dict({**model.state_dict(), **eng.state_dict("decoder.")})
            if eng.binary_grid is not None:      # (save_checkpoint refreshes the DensityGrid from the weights it saves)
                grid.grid, grid.binary_grid = eng.grid.clone(), eng.binary_grid.clone()

        def draw(counter):
            # every rank forms and compacts rays [first_ray, first_ray + local_batch) of the step's global batch
            if fused_batch:
                return train_set.train_batch_compact(local_batch, n_samples, near, far, eng.bg, seed, counter, eng.binary_grid, eng.bound,
                                                     first_ray=first_ray)
            o, d, target, _ = train_set.train_batch(local_batch, n_samples, near, far, eng.bg, seed=seed, counter=counter,
                                                    first_ray=first_ray)
            return o, d, target, eng.prepare_batch(o, d, n_samples, first_ray=first_ray)

        active, ahead = 1.0, []
        for step in range(1, train_iters + 1):
            through_grid = eng.binary_grid is not None
            if through_grid:
                # the batch was drawn and compacted ONE step ahead: its active count arrived while the previous step computed
                if not ahead:
                    ahead.append(draw(step))
                rays_o, rays_d, target, prepared = ahead.pop()
                if step < train_iters:
                    ahead.append(draw(step + 1))
                loss = eng.train_step(rays_o, rays_d, target, n_samples, prepared=prepared, sync_grads_async=sync_async)
            else:
                rays_o, rays_d, target, z = train_set.train_batch(local_batch, n_samples, near, far, eng.bg, seed=seed, counter=step,
                                                                  first_ray=first_ray)
                loss = eng.train_step(rays_o, rays_d, target, n_samples, z=z, sync_grads_async=sync_async)
            if step % log_every == 0:
                loss_val = parallel.mean_over_ranks(loss).item()
                psnr = compute_psnr(loss_val)
                say(f">>> Step {step}/{train_iters} | Loss {loss_val:.6f} | PSNR {psnr:.2f} dB"
                    + (f" | Skip: {(1 - active) * 100:.1f}%" if through_grid else " | dense"))
                if tb is not None:
                    tb.log_scalar("Train/Loss", loss_val, step)
                    tb.log_scalar("Train/PSNR", psnr, step)
            if grid_refresh_due(step, train_iters, warm, stop):
                ratio = eng.update_grid()       # (replicated: every rank holds the same weights)
                ahead.clear()                   # the waiting batch was compacted against the previous grid
                if ratio > 0.0:
                    active = ratio
                    say(f">>> Density grid: refreshed after step {step} ({ratio * 100:.1f} % of the cells occupied)")
                else:
                    say(f">>> Density grid: no cell above the threshold after step {step}; the previous grid stays"
                        + ("" if eng.binary_grid is not None else " (dense steps go on)"))
            if save_every and step % save_every == 0 and main_rank:
                sync_model()
                save_checkpoint(os.path.join(ckpt_dir, f"model_step_{step:06d}.pth"))
        sync_model()
        if main_rank:
            save_checkpoint(os.path.join(ckpt_dir, "model_final.pth"))
            tb.close()
    elif use_engine:
        from project_nerf_amd.engine import VanillaNerfEngine
        tb = TensorBoardLogger(os.path.join(log_dir, "tensorboard")) if main_rank else None
        eng = VanillaNerfEngine(params=dec.flat_parameters(), device=str(device), lr=lr, near=near, far=far, white_bkgd=white_bkgd,
                                world_size=world)
        sync_async = parallel.allreduce_sum_async if world > 1 else None

        def sync_model():
            model.load_state_dict({**model.state_dict(), **eng.state_dict("decoder.")})

        for step in range(1, train_iters + 1):
            # every rank forms rays [first_ray, first_ray + local_batch) of the step's global batch (same seed and counter)
            rays_o, rays_d, target, z = train_set.train_batch(local_batch, n_samples, near, far, eng.bg, seed=cfg.get("seed", 0),
                                                              counter=step, first_ray=first_ray)
            loss = eng.train_step(rays_o, rays_d, target, n_samples, z=z, sync_grads_async=sync_async)
            if step % log_every == 0:
                loss_val = parallel.mean_over_ranks(loss).item()          # mean of the shards' means = the global batch's loss
                psnr = compute_psnr(loss_val)
                say(f">>> Step {step}/{train_iters} | Loss {loss_val:.6f} | PSNR {psnr:.2f} dB")
                if not bool((eng.grads != 0).any()):
                    # the reference's density head is a bare ReLU (src/decoders.py:78): once every density of the batches is
                    # zero, every gradient is exactly zero and the run cannot recover
                    say(">>> WARNING: all gradients are exactly zero -- every density of the batch is zero (dead ReLU density "
                        "head); this run will not recover: restart with another `seed:` in the YAML")
                if tb is not None:
                    tb.log_scalar("Train/Loss", loss_val, step)
                    tb.log_scalar("Train/PSNR", psnr, step)
            if save_every and step % save_every == 0 and main_rank:
                sync_model()
                save_checkpoint(os.path.join(ckpt_dir, f"model_step_{step:06d}.pth"))
        sync_model()
        if main_rank:
            save_checkpoint(os.path.join(ckpt_dir, "model_final.pth"))
            tb.close()
    elif p2_eng is not None:
        tb = TensorBoardLogger(os.path.join(log_dir, "tensorboard"))
        eng = p2_eng

        def sync_model():
            eng.copy_to_model(model)

        for step in range(1, train_iters + 1):
            rays_o, rays_d, target, z = train_set.train_batch(local_batch, n_samples, near, far, eng.bg, seed=cfg.get("seed", 0),
                                                              counter=step, first_ray=first_ray)
            loss = eng.train_step(rays_o, rays_d, target, n_samples, z=z)
            if step % log_every == 0:
                loss_val = loss.item()
                psnr = compute_psnr(loss_val)
                say(f">>> Step {step}/{train_iters} | Loss {loss_val:.6f} | PSNR {psnr:.2f} dB")
                if not bool((eng.grads != 0).any()):
                    # the dead density head of the default engine's loop above
                    say(">>> WARNING: all gradients are exactly zero -- every density of the batch is zero (dead ReLU density "
                        "head); this run will not recover: restart with another `seed:` in the YAML")
                tb.log_scalar("Train/Loss", loss_val, step)
                tb.log_scalar("Train/PSNR", psnr, step)
            if save_every and step % save_every == 0:
                sync_model()
                save_checkpoint(os.path.join(ckpt_dir, f"model_step_{step:06d}.pth"))
        sync_model()
        save_checkpoint(os.path.join(ckpt_dir, "model_final.pth"))
        tb.close()
    elif not args.eval_only:
        tb = TensorBoardLogger(os.path.join(log_dir, "tensorboard")) if main_rank else None
        optimizer = torch.optim.Adam(model.parameters(), lr=lr)
        bg = torch.ones(3, device=device) if white_bkgd else torch.zeros(3, device=device)
        model.train()
        for step in range(1, train_iters + 1):
            # module path: every rank draws the same global batch (same torch seed) and keeps its shard
            rays_o, rays_d, rgba = train_set.sample_random_rays(local_batch * world, device)
            rays_o, rays_d, rgba = (t[first_ray:first_ray + local_batch].contiguous() for t in (rays_o, rays_d, rgba))
            target = _target(rgba, bg)
            pred, _, _ = render_rays(model, rays_o, rays_d, near, far, n_samples, True, white_bkgd=white_bkgd)
            loss = torch.nn.functional.mse_loss(pred, target)
            optimizer.zero_grad()
            loss.backward()
            parallel.allreduce_mean_grads_(list(model.parameters()))
            optimizer.step()
            if step % log_every == 0:
                loss_val = parallel.mean_over_ranks(loss).item()
                psnr = compute_psnr(loss_val)
                say(f">>> Step {step}/{train_iters} | Loss {loss_val:.6f} | PSNR {psnr:.2f} dB")
                if tb is not None:
                    tb.log_scalar("Train/Loss", loss_val, step)
                    tb.log_scalar("Train/PSNR", psnr, step)
            if save_every and step % save_every == 0 and main_rank:
                save_checkpoint(os.path.join(ckpt_dir, f"model_step_{step:06d}.pth"))
        if main_rank:
            save_checkpoint(os.path.join(ckpt_dir, "model_final.pth"))
            tb.close()

    model.eval()
    if grid is not None and not (args.eval_only and grid_loaded) and (args.eval_only or not main_rank):
        refresh_grid()          # (after training, rank 0 refreshed it when it wrote the final checkpoint)

    def render_grid_band(o, d):
        """a band of rows through the occupancy grid as one launch chain (renderer.render_rays_nerf_grid_chain)"""
        rows, width = o.shape[0], o.shape[1]
        if rows * width == 0:
            return o.new_zeros(0, width, 3)
        return render_rays_nerf_grid_chain(model, o.reshape(-1, 3), d.reshape(-1, 3), near, far, render_n_samples, grid, white_bkgd,
                                           chunk)[0].view(rows, width, 3)

    psnrs = []
    n_eval = len(test_set) if args.render_n in (None, -1) else min(args.render_n, len(test_set))
    with torch.no_grad():
        for idx in range(n_eval):
            rays_o, rays_d, target = test_set.get_image_rays(idx, device)
            # row bands over the ranks, gathered on rank 0 (one rank: the whole frame)
            if grid is not None:         # only the active samples reach the decoder; no host read of their count
                pred = parallel.render_row_bands(render_grid_band, rays_o, rays_d)
            elif p2_eng is not None:     # single rank: the whole frame through the engine's inference chain
                pred = p2_eng.render_image(rays_o, rays_d, render_n_samples, chunk)
            else:
                pred = parallel.render_row_bands(
                    lambda o, d: render_image_safe(render_image, model, o, d, near, far, render_n_samples, chunk, white_bkgd), rays_o, rays_d)
            if not main_rank:
                continue
            pred = torch.clamp(pred, 0.0, 1.0)
            psnrs.append(compute_psnr_torch(pred, target))
            try:
                from PIL import Image
                Image.fromarray((pred.cpu().numpy() * 255 + 0.5).astype(np.uint8)).save(
                    os.path.join(render_dir, f"test_{idx:03d}.png"))
            except ImportError:
                pass
    avg = float(np.mean(psnrs)) if psnrs else 0.0
    say(f">>> Test PSNR: {avg:.2f} dB")
    return avg


def run_part1(cfg, args):
    """2-D image fit (reference run.py:30-237), single configuration: HIP Fourier features + MLP."""
    from PIL import Image
    if not args.image:
        raise ValueError("Part 1 requires --image")
    if not torch.cuda.is_available():
        raise RuntimeError("a HIP device is required")
    device = torch.device("cuda")
    size = cfg.get("image_size", 400)
    img = Image.open(args.image).convert("RGB")
    scale = min(size / img.width, size / img.height)
    img = img.resize((int(img.width * scale), int(img.height * scale)), Image.LANCZOS)
    arr = np.array(img) / 255.0
    h, w, _ = arr.shape
    coords = torch.stack(torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij"), -1).reshape(-1, 2).to(device)
    gt = torch.tensor(arr.reshape(-1, 3), dtype=torch.float32, device=device)
    pick = lambda v: v[0] if isinstance(v, (list, tuple)) else v
    cfg = dict(cfg, L_embed=pick(cfg["L_embed"]), hidden_dim=pick(cfg["hidden_dim"]), num_layers=pick(cfg.get("num_layers", 3)),
               use_positional_encoding=pick(cfg.get("use_positional_encoding", True)))
    model = NeuralField(cfg).to(device)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location=device)["model_state_dict"], strict=False)
    log_dir = os.path.join(cfg.get("log_dir", "output/"), "part1", os.path.splitext(os.path.basename(args.image))[0])
    os.makedirs(log_dir, exist_ok=True)
    engine = None
    if cfg.get("engine", False) and not args.eval_only:
        # fused HIP training engine (project-nerf_amd/part1.py); a shape it is not compiled for keeps the module path
        from project_nerf_amd import part1
        why = part1.supported(cfg)
        if why is None:
            engine = part1.Part1Engine(cfg, device="cuda", lr=cfg["learning_rate"])
            engine.load_from_model(model)
            print(f">>> Part 1 on the fused HIP engine ({engine.params.numel()} parameters)")
        else:
            print(f">>> Part 1 engine not used: {why}; training on the module path")
    if engine is not None:
        bs = cfg.get("batch_size")
        for epoch in range(1, cfg["epochs"] + 1):
            idx = None if bs is None else torch.randint(0, coords.shape[0], (bs,), device=device)
            loss = engine.train_step(coords, gt, idx)
            if epoch % cfg.get("log_every", 100) == 0:
                print(f">>> Epoch {epoch}/{cfg['epochs']} | Loss {loss.item():.6f} | PSNR {compute_psnr(loss.item()):.2f} dB")
        engine.copy_to_model(model)
        torch.save({"model_state_dict": model.state_dict(), "config": cfg}, os.path.join(log_dir, "model_final.pth"))
    elif not args.eval_only:
        opt = torch.optim.Adam(model.parameters(), lr=cfg["learning_rate"])
        bs = cfg.get("batch_size")
        for epoch in range(1, cfg["epochs"] + 1):
            idx = slice(None) if bs is None else torch.randint(0, coords.shape[0], (bs,), device=device)
            loss = torch.nn.functional.mse_loss(model(coords[idx]), gt[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
            if epoch % cfg.get("log_every", 100) == 0:
                print(f">>> Epoch {epoch}/{cfg['epochs']} | Loss {loss.item():.6f} | PSNR {compute_psnr(loss.item()):.2f} dB")
        torch.save({"model_state_dict": model.state_dict(), "config": cfg}, os.path.join(log_dir, "model_final.pth"))
    with torch.no_grad():
        pred = (engine.predict(coords) if engine is not None else model(coords)).clamp(0, 1)
    psnr = compute_psnr(torch.nn.functional.mse_loss(pred, gt).item())
    Image.fromarray((pred.cpu().numpy().reshape(h, w, 3) * 255 + 0.5).astype(np.uint8)).save(os.path.join(log_dir, "final.png"))
    print(f">>> Final PSNR: {psnr:.2f} dB")
    return psnr


def run_part2_instant(cfg, args):
    """Instant-NGP style training (reference run.py:396-900)."""
    from project_nerf_amd.instant import run_instant
    return run_instant(cfg, args)


def run_part4(cfg, args):
    """Dual-hash dynamic NeRF (reference run.py:1562-2331)."""
    from project_nerf_amd.dynamic import run_dynamic
    return run_dynamic(cfg, args)


def main():
    ap = argparse.ArgumentParser(description="MI355X-native NeRF (CLI of CV-Project2025/Project-NeRF)")
    ap.add_argument("--image", type=str, default=None)
    ap.add_argument("--data_dir", type=str, default=None)
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint", type=str, default=None)
    ap.add_argument("--eval_only", action="store_true")
    ap.add_argument("--render_n", type=int, default=None)
    ap.add_argument("--render_chunk", type=int, default=None)
    args = ap.parse_args()
    with open(args.config, "r", encoding="utf-8") as f:
        cfg = yaml.safe_load(f)
    mode = cfg.get("mode")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        # one process per GPU (torch.distributed.run): the process group -- RCCL over xGMI -- and the device are chosen
        # BEFORE anything touches the GPU; replicas must start from the same weights and draw the same global batches,
        # so a data-parallel run is always seeded (`seed:` in the YAML, default 0)
        from project_nerf_amd import parallel
        parallel.init_distributed("cuda")
        if cfg.get("seed") is None:          # also a YAML `seed: null`
            cfg["seed"] = 0
    if cfg.get("deterministic") or os.environ.get("NERF_DETERMINISTIC", "") not in ("", "0"):
        # every sum whose order would depend on scheduling takes an ordered form: two runs of the same command give the same
        # bits (include/nerf_hip.h, option "deterministic"; costs 0.1-0.3 ms per Instant / Part 4 step)
        from project_nerf_amd import ops
        ops.set_deterministic(True)
    if cfg.get("seed") is not None:        # extension: the reference seeds nothing; a YAML `seed` makes a run repeatable
        torch.manual_seed(int(cfg["seed"]))
        np.random.seed(int(cfg["seed"]))
        import random
        random.seed(int(cfg["seed"]))
    if mode == "part1_fourier":
        run_part1(cfg, args)
    elif mode == "part2_nerf":
        run_part2(cfg, args)
    elif mode == "part2_instant":
        run_part2_instant(cfg, args)
    elif mode in ("part3", "part4"):
        run_part4(cfg, args)           # one loop for both dynamic modes (project-nerf_amd/dynamic.py)
    else:
        raise ValueError(f"mode {mode!r} is not built (part1_fourier, part2_nerf, part2_instant, part3, part4 are); see DESIGN.md")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
