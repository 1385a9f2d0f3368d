#!/usr/bin/env python3
"""Headline benchmark: 512x512 images/sec @ 50 DDIM steps, seg-ControlNet + CFG (BASELINE.json configs[2], "C3").

One "step" = one complete 50-step DDIM sampling (eta 0, CFG as one 2B batch) of this rank's 16 prompts through
SD-v1.5 UNet + one ControlNet, latent 64x64, hint 512x512, inputs already resident in HBM.  Weak scaling:
every rank samples its own 16 prompts (global x_T / contexts / hints are generated once and sliced), no
collective inside the loop; frozen weights are generated on rank 0 and broadcast over RCCL before timing.

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself (one child
`python -m torch.distributed.run --nproc-per-node N ... bench.py ...`, before this process touches the GPU), relays rank
0's JSON line and exits with the children's status.  Under an external torchrun the environment decides.

Prints ONE JSON line on rank 0 (contract in the task statement) with `roofline` (dominant kernel = the
implicit-GEMM family, timed with HIP events on the launch stream inside the timed region).  A plain run sets up, warms
up, times --steps samplings and prints that line; `--full` adds the measurements the headline does not need, each after
the timed region: `cpu_baseline` (the CPU oracle on a bounded sample of the same workload, rank 0) and
`first_stage_decode` (the VAE decode of the sampled latents).

`--dump-outputs DIR` writes what the last timed sampling returned (the latents and the sampler's intermediates, all
ranks gathered) as DIR/<name>.npy in float32; the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

PROMPTS_PER_GPU = 16
DDIM_STEPS = 50
CFG_SCALE = 9.0          # reference stage-B default: scripts/txt2img_fgdm_inference.py:292, controlnet/initialize_cn.py:74
LATENT = 64
TFLOP_PER_IMAGE = 107.20  # BASELINE.md section 3, config C3 (hint block once per image)
PEAK_TFLOPS = 2500.0      # dense fp16 MFMA, MI355X_MICROARCH.md
PROFILE_TAG = 'r04'       # profiles/<tag>_pmc_traffic.json / _trace_summary.json: offline measurements quoted (and labelled) in the line
DUMP_BUDGET = 60 * 10**6  # bytes of arrays written by --dump-outputs at most (64 MB with room for the .npy headers)


def log(msg):
    """progress on stderr (stdout carries exactly one JSON line)"""
    print(f'[bench] {msg}', file=sys.stderr, flush=True)


def build_model(rank, world, device, first_stage=True, n_controlnets=1, force_bcast=False):
    """ControlLDM mirror (reference API) over the HIP engine; frozen weights are generated on rank 0 only and
    shipped with ONE RCCL broadcast of a flat buffer (fp16 where the engine keeps fp16; fgdm_amd/dist.py)."""
    from fgdm_amd import dist as fd, models, synth
    t0 = time.time()
    model = models.ControlLDM(None, n_controlnets=n_controlnets, device=torch.cuda.current_device(),
                              first_stage_config=True if first_stage else None)
    shapes = model.engine.param_shapes()
    timing = {}
    sd, flat = fd.broadcast_weights(shapes, synth.make_tensor, rank, world, device, timing, force=force_bcast)
    missing, _ = model.load_state_dict(sd, strict=True)
    assert not missing
    n_params = sum(int(np.prod(s)) for s in shapes.values())
    del sd, flat
    torch.cuda.empty_cache()
    timing['load_s'] = time.time() - t0
    return model, n_params, timing


def launch_ranks(n, argv):
    """Start n ranks of this script on this node (one process per GPU) and wait for them.  Runs BEFORE anything in
    this process has touched the GPU; the children are fresh processes, nothing is re-exec'ed."""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + argv
    log(f'--gpus {n}: starting {n} ranks: {" ".join(cmd)}')
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')      # dmabuf IPC (RCCL across processes on this pool)
    env.setdefault('OMP_NUM_THREADS', str(max(1, (os.cpu_count() or 8) // n)))
    return subprocess.run(cmd, env=env).returncode


class DryRunModel:
    """--dry-run: CPU rehearsal of the launcher / sharding / broadcast / timing plumbing with the analytic stand-in model
    and the torch stand-ins of the sampler kernels that the CPU test-suite uses (tests/test_samplers_host.py,
    tests/kernel_stubs.py).  Nothing of the product is measured; the JSON line says "dry_run": true."""

    @staticmethod
    def build(rank, world):
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import kernel_stubs
        from fgdm_amd import dist as fd, models, samplers, synth
        from test_samplers_host import AnalyticLDM
        samplers._k = kernel_stubs
        models._k = kernel_stubs
        shapes = {'model.diffusion_model.time_embed.0.weight': (1280, 320), 'model.diffusion_model.time_embed.0.bias': (1280,),
                  'model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight': (320, 320)}
        timing = {}
        make = synth.make_tensor if rank == 0 else (lambda k, s: np.full(s, np.nan, np.float32))
        sd, _ = fd.broadcast_weights(shapes, make, rank, world, 'cpu', timing)
        for k, s in shapes.items():      # every rank must hold rank 0's bytes
            want = torch.from_numpy(synth.make_tensor(k, s)).to(sd[k].dtype)
            assert torch.equal(sd[k], want), k
        timing['load_s'] = 0.0
        return AnalyticLDM(), sum(int(np.prod(s)) for s in shapes.values()), timing


def cpu_baseline():
    """CPU oracle (port of the reference's PyTorch-CPU path) on a bounded sample of the SAME workload:
    one prompt's CFG pair = 2 x (ControlNet + ControlledUnet) at 64x64 latent, hint 512x512, fp32."""
    from fgdm_amd import synth
    from oracle import arch, nn as onn
    cfg = dict(in_channels=4, out_channels=4, model_channels=320, attention_resolutions=(4, 2, 1),
               num_res_blocks=2, channel_mult=(1, 2, 4, 4), num_heads=8, context_dim=768)
    # host cores this process may use: the GPU box gives a CPU share of 16 per GPU whatever os.cpu_count() says
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, int(os.environ.get('FGDM_CPU_BASELINE_THREADS', '16'))))
    torch.set_num_threads(cores)
    log(f'cpu_baseline: oracle ControlNet+UNet CFG pair on {cores} host threads ...')
    p = {}
    for pre, shapes in (('model.diffusion_model.', arch.unet_param_shapes(cfg, adapter=False)),
                        ('control_model.', arch.controlnet_param_shapes(cfg))):
        for k, s in shapes.items():
            p[pre + k] = torch.from_numpy(synth.make_tensor(pre + k, s))
    x = torch.from_numpy(synth.latents(1, LATENT, LATENT)).repeat(2, 1, 1, 1)
    ctx = torch.cat([torch.from_numpy(synth.context(1, seed=44)), torch.from_numpy(synth.context(1, seed=43))])
    hint = torch.from_numpy(synth.hint(1, 512)).repeat(2, 1, 1, 1)
    t = torch.full((2,), 981, dtype=torch.long)
    times = []
    with torch.no_grad():
        for i in range(3):
            t0 = time.time()
            onn.control_ldm_apply(p, cfg, x, t, ctx, [hint])
            times.append(time.time() - t0)
            log(f'cpu_baseline: evaluation {i} took {times[-1]:.1f} s')
    sec = float(np.mean(times[1:]))            # first call = warm-up
    return {'value': 1.0 / (DDIM_STEPS * sec), 'unit': 'images/s', 'cores': cores, 'kind': 'port',
            'sample': f'2 timed CFG-pair evaluations (B=2: uncond+cond) of ControlNet+UNet @64x64, hint 512^2, '
                      f'fp32 torch-CPU oracle, {sec:.2f} s each, extrapolated x{DDIM_STEPS} DDIM steps for one image',
            'sec_per_cfg_pair_eval': sec}


def dump_outputs(d, out, inter, rank, world, use_dist):
    """np.save the last timed sampling's result as d/<name>.npy (float32): `samples` and the sampler's intermediates
    `x_inter_<i>` / `pred_x0_<i>`, the batches of all ranks gathered in rank order.  Above DUMP_BUDGET bytes in all, the
    same fixed, seeded subset of batch rows is kept in every array (and listed in `rows.npy`)."""
    from fgdm_amd import dist as fd
    arrays = {'samples': out}
    for k in ('x_inter', 'pred_x0'):
        arrays.update({f'{k}_{i}': t for i, t in enumerate(inter[k])})
    arrays = {k: (fd.gather_latents(v, rank, world) if use_dist else v).float().cpu().numpy() for k, v in arrays.items()}
    if rank != 0:
        return
    os.makedirs(d, exist_ok=True)
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_BUDGET:
        n = arrays['samples'].shape[0]
        keep = max(1, n * DUMP_BUDGET // total)
        rows = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrays = {k: v[rows] for k, v in arrays.items()}
        arrays['rows'] = rows.astype(np.float64)
    for k, v in arrays.items():
        np.save(os.path.join(d, k + '.npy'), v)
    log(f'outputs of the last timed step written to {d}: {", ".join(sorted(arrays))}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--prompts', type=int, default=PROMPTS_PER_GPU, help='prompts per GPU')
    ap.add_argument('--ddim-steps', type=int, default=DDIM_STEPS)
    ap.add_argument('--full', action='store_true',
                    help='after the timed region, also measure what the headline does not need: the CPU baseline and the '
                         'first-stage (VAE) decode')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--controlnets', type=int, default=1,
                    help='control models per UNet (1 = the metric\'s config C3; 2 / 3 = BASELINE configs C4 / C5, use --prompts 8; 0 = the plain UNet, C2)')
    ap.add_argument('--no-first-stage', action='store_true',
                    help='with --full: skip the VAE decode that follows the timed region (PMC passes: counters then cover the '
                         'path only)')
    ap.add_argument('--profile-stride', type=int, default=31,
                    help='HIP-event bracket every n-th kernel launch of the timed region (coprime with the 830 launches per '
                         'evaluation, so every layer shape is sampled uniformly); 1 = every launch.  Two event packets leave a ~6 us '
                         'hole in the queue: at stride 7 they cost 0.3-0.8 %% of the step (profiles/r04_ab_profile_stride.txt)')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'],
                    help='torch.distributed backend: nccl (= RCCL over xGMI, the product) or gloo (CPU rehearsal with --dry-run)')
    ap.add_argument('--twin-streams', action='store_true',
                    help='FGDM_TWIN_STREAMS=1: the ControlNets run on a second HIP stream next to the UNet encoder (DESIGN.md section 4.3). '
                         'Off by default: launches of the two streams overlap, so per-launch durations (the roofline object, rocprof '
                         'kernel statistics) stop being exclusive device time; the JSON line says "twin_streams": true')
    ap.add_argument('--dump-latents', default=None,
                    help='after timing, gather the last sampling\'s latents of all ranks (all_gather) and np.save them here (tests: '
                         'N ranks must reproduce the 1-rank result of the same global batch bit for bit)')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='after timing, write what the last timed sampling returned (latents and intermediates, all ranks) '
                         'as DIR/<name>.npy, float32')
    ap.add_argument('--dry-run', action='store_true',
                    help='CPU rehearsal of the N-rank plumbing with an analytic stand-in model (tests); measures nothing')
    a = ap.parse_args()
    if a.steps < 1:
        ap.error('--steps must be at least 1')
    first_stage = a.full and not a.no_first_stage

    if a.twin_streams:
        os.environ['FGDM_TWIN_STREAMS'] = '1'          # read by fgdm_create; inherited by the ranks of --gpus N
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(launch_ranks(a.gpus, sys.argv[1:]))       # nothing has touched the GPU yet
    # stdout carries exactly ONE line, the JSON: native libraries write there too (RCCL prints a version banner on the first
    # collective), so file descriptor 1 is pointed at stderr for the whole run and the JSON goes to a saved copy of it
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    def emit(obj):
        os.write(json_fd, (json.dumps(obj) + '\n').encode())

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if a.gpus != world:
        print(f'warning: --gpus {a.gpus} != WORLD_SIZE {world}; the launcher decides: {world} ranks', file=sys.stderr)
    if a.dry_run and a.backend != 'gloo':
        sys.exit('--dry-run is a CPU rehearsal: use --backend gloo')
    if a.backend == 'gloo' and not a.dry_run:
        sys.exit('--backend gloo only exists for --dry-run: the product path needs the GPUs (there is no CPU fallback)')
    dev = 'cpu' if a.dry_run else 'cuda'
    if not a.dry_run:
        torch.cuda.set_device(local)
    import torch.distributed as dist
    # FGDM_BENCH_FORCE_DIST=1: take the collective code paths (process group, broadcast, barrier, all_reduce, all_gather) even
    # with ONE rank -- the only way to run them over RCCL on a one-GPU box before the 8-GPU driver run does
    use_dist = world > 1 or os.environ.get('FGDM_BENCH_FORCE_DIST') == '1'
    if use_dist:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29513')
        kw = {'device_id': torch.device('cuda', local)} if a.backend == 'nccl' else {}
        dist.init_process_group(a.backend, rank=rank, world_size=world, **kw)

    if os.environ.get('FGDM_BENCH_FAIL_RANK') == str(rank):     # tests: a dying rank must fail the whole launch
        sys.exit(3)
    from fgdm_amd import synth
    from fgdm_amd import samplers
    if a.dry_run:
        model, n_params, wt = DryRunModel.build(rank, world)
        engine = None
        sampler = samplers.DDIMSampler(model)
    else:
        model, n_params, wt = build_model(rank, world, dev, first_stage=first_stage, n_controlnets=a.controlnets,
                                          force_bcast=use_dist)
        engine = model.engine
        sampler = samplers.ControlDDIMSampler(model)       # drop-in for controlnet/cldm/ddim_hacked.py:DDIMSampler
    load_s = wt['load_s']

    npg = a.prompts
    N = npg * world
    sl = slice(rank * npg, (rank + 1) * npg)
    lat = 8 if a.dry_run else LATENT
    x_T = torch.from_numpy(synth.latents(N, lat, lat, seed=42)[sl]).to(dev)
    cond0 = torch.from_numpy(synth.context(N, seed=43)[sl]).to(dev)
    uncond0 = torch.from_numpy(synth.context(N, seed=44)[sl]).to(dev)
    hints0 = [torch.from_numpy(synth.hint(N, 8 * lat, seed=45 + k)[sl]).to(dev) for k in range(a.controlnets)]

    def one_step():
        # every sampling gets FRESH hint / context tensors, as a new batch of images would: the ControlNet hint block
        # (once per image) and the K/V projections of the conditioning (once per sample() call) are therefore computed
        # inside the timed region -- the engine's caches are keyed on tensor identity
        hints = [h.clone() for h in hints0]
        cond, uncond = cond0.clone(), uncond0.clone()
        if a.dry_run:
            return sampler.sample(a.ddim_steps, npg, (4, lat, lat), conditioning=cond, verbose=False, eta=0.0, x_T=x_T,
                                  unconditional_guidance_scale=CFG_SCALE, unconditional_conditioning=uncond)
        # the call the reference makes at controlnet/initialize_cn.py:86-96 (guess_mode=False: control on both branches)
        # --controlnets 0 (the plain UNet, BASELINE configs[1]): c_concat = None as in cldm.py:840-842
        c_cond = {'c_crossattn': [cond], 'c_concat': hints if hints else None}
        c_uncond = {'c_crossattn': [uncond], 'c_concat': hints if hints else None}
        return sampler.sample(a.ddim_steps, npg, (4, LATENT, LATENT), c_cond, verbose=False, eta=0.0, x_T=x_T,
                              unconditional_guidance_scale=CFG_SCALE, unconditional_conditioning=c_uncond)

    def barrier():
        if use_dist:
            dist.barrier()
        if not a.dry_run:
            torch.cuda.synchronize()

    if rank == 0:
        log(f'weights ready ({n_params / 1e9:.2f} G params, {load_s:.1f} s); warm-up x{a.warmup} ...')
    for _ in range(a.warmup):
        one_step()
    barrier()
    if rank == 0:
        log(f'timing {a.steps} step(s) of {a.ddim_steps} DDIM steps x {npg} prompts per GPU ...')
    if engine is not None:
        engine.profile_begin(a.profile_stride)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out, inter = one_step()
    if not a.dry_run:
        torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0        # this rank's own time (before it waits for the others)
    barrier()
    dt = time.perf_counter() - t0
    prof = engine.profile_end() if engine is not None else None
    per_rank = [npg * a.steps / dt_own]
    if use_dist:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        rates = [torch.zeros(1, dtype=torch.float64, device=dev) for _ in range(world)]
        dist.all_gather(rates, torch.tensor([npg * a.steps / dt_own], dtype=torch.float64, device=dev))
        per_rank = [float(r.item()) for r in rates]
    assert torch.isfinite(out).all(), 'non-finite latents'
    if a.dump_latents:
        from fgdm_amd import dist as fd
        allx = fd.gather_latents(out, rank, world) if use_dist else out
        if rank == 0:
            np.save(a.dump_latents, allx.float().cpu().numpy())
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, out, inter, rank, world, use_dist)
    if a.dry_run:
        if rank == 0:
            emit({'metric': '512x512 images/sec @ 50 DDIM steps, seg-ControlNet+CFG', 'dry_run': True, 'value': None,
                              'unit': 'images/s', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup, 'backend': a.backend,
                              'ms_per_step': dt / a.steps * 1e3, 'scaling': 'weak', 'per_rank_images_per_s': per_rank,
                              'weights': {'params': n_params, 'bcast_s': wt.get('bcast_s'), 'bcast_bytes': wt.get('bcast_bytes')},
                              'config': {'workload': 'DRY RUN: analytic stand-in model on CPU, launcher/shard/broadcast rehearsal only',
                                         'prompts_per_gpu': npg}})
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return
    # outside the timed region (VAE decode excluded from the metric, reported separately):
    # decode_first_stage of this rank's latents to 512x512 images
    dec_s = None
    if first_stage:
        img = model.decode_first_stage(out)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        img = model.decode_first_stage(out)
        torch.cuda.synchronize()
        dec_s = time.perf_counter() - t1
        assert tuple(img.shape) == (npg, 3, 8 * LATENT, 8 * LATENT) and torch.isfinite(img).all()

    if rank == 0:
        # HBM traffic per launch of the dominant kernel family: measured offline with rocprofv3 PMC passes
        # (tools/pmc_summary.py -> profiles/pmc_traffic.json); null when no measurement is committed
        # Both are OFFLINE measurements of the default command (C3, 16 prompts, 50 steps, one stream), committed under profiles/
        # with the commit they were taken at (`source`); they describe no other configuration, so every other run reports null
        # here and the live HIP-event figures stand alone.
        is_traced_cmd = (a.controlnets == 1 and npg == 16 and a.ddim_steps == DDIM_STEPS and world == 1
                         and os.environ.get('FGDM_TWIN_STREAMS') != '1')
        traffic, traffic_src = None, None
        frac_trace = None
        if is_traced_cmd:
            try:
                pj = json.load(open(os.path.join(ROOT, 'profiles', PROFILE_TAG + '_pmc_traffic.json')))
                traffic = pj['igemm']['hbm_bytes_per_launch']
                traffic_src = f"profiles/{PROFILE_TAG}_pmc_traffic.json @ {pj.get('_source_commit', 'unknown commit')} (offline rocprofv3 --pmc passes, not this run)"
            except Exception:
                pass
            # the same family's time from the committed rocprofv3 kernel trace of this command (tools/trace_summary.py: the last
            # sampling pass, cut by kernel names): no event packets around the launches, so it reads a few percent below the
            # live HIP-event brackets
            try:
                tj = json.load(open(os.path.join(ROOT, 'profiles', PROFILE_TAG + '_trace_summary.json')))
                fam = tj['families']['igemm']
                frac_trace = {'igemm_ms_per_sampling': fam['ms'], 'launches': fam['launches'],
                              'source': f"profiles/{PROFILE_TAG}_trace_summary.json @ {tj.get('_source_commit', 'unknown commit')} (offline, not this run)",
                              'note': 'rocprofv3 --kernel-trace of `bench.py --steps 1 --warmup 1`, last sampling pass (first '
                                      'k_timestep_embed .. last k_ddim_step); achieved = the pass\'s algorithmic igemm FLOPs / '
                                      'this time is reported in DESIGN.md section 5'}
            except Exception:
                pass
        images = N * a.steps
        value = images / dt
        # 2*50*(803.27 + k*268.57) + k*14.72 GFLOP per image
        tflop_per_image = TFLOP_PER_IMAGE if a.controlnets == 1 else (100 * (803.27 + a.controlnets * 268.57) + a.controlnets * 14.72) / 1e3
        # ... of which the CFG-shared network prefix (conv_in, first ResBlock, first SpatialTransformer up to its cross-attention:
        # 40.8 GFLOP per net and shared row) is EXECUTED once per pair instead of twice
        exec_tflop_per_image = tflop_per_image - 2 * DDIM_STEPS * (1 + a.controlnets) * 0.0408 / 2
        ig = prof['igemm']
        achieved = ig['work'] / (ig['ms'] * 1e-3) / 1e12 if ig['ms'] > 0 else 0.0
        res = {
            'metric': '512x512 images/sec @ 50 DDIM steps, seg-ControlNet+CFG',
            'value': value, 'unit': 'images/s', 'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup,
            'ms_per_step': dt / a.steps * 1e3, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': 'f16', 'data': 'synthetic',
            'config': {'workload': ('BASELINE configs[2] (C3): SD-v1.5 UNet + seg-ControlNet, hint 512x512, ' if a.controlnets == 1 else
                                    f'NOT the metric\'s config: SD-v1.5 UNet + {a.controlnets} ControlNets (summed residuals), hints 512x512, ')
                                   +
                                   f'{npg} prompts per GPU, {a.ddim_steps} DDIM steps eta=0, CFG {CFG_SCALE} '
                                   'as one 2B batch, latent 4x64x64, through the drop-in ControlLDM.apply_model + '
                                   'DDIMSampler.sample API; synthetic weights/latents/contexts/hints',
                       'prompts_per_gpu': npg, 'ddim_steps': a.ddim_steps, 'cfg_scale': CFG_SCALE,
                       'parallelism': f'prompt-shard x{world}, RCCL weight broadcast only'},
            'roofline': {'bound': 'mfma', 'achieved': achieved, 'peak': PEAK_TFLOPS, 'unit': 'TFLOP/s',
                         'frac': achieved / PEAK_TFLOPS, 'traffic': traffic, 'traffic_source': traffic_src,
                         'traffic_unit': 'HBM bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE, rocprofv3)',
                         'algorithmic_bytes_per_launch': ig['bytes'] / max(ig['launches'], 1),
                         'kernel': 'igemm_kernel<*> (implicit-GEMM conv3x3/conv1x1/linear family)',
                         'timed_launches': ig['launches'], 'launch_sampling_stride': a.profile_stride,
                         'avg_launch_us': ig['ms'] * 1e3 / max(ig['launches'], 1),
                         'algorithmic_tflop_per_launch': ig['work'] / max(ig['launches'], 1) / 1e12,
                         'rocprof_trace': frac_trace},
            'exact_shortcuts': ['ControlNet hint block evaluated once per image batch, INSIDE the timed region (t-independent; the '
                                'reference recomputes it every call)',
                                'to_k/to_v of the loop-invariant context projected once per sample() call, inside the timed region',
                                'CFG batch cat([x]*2): network prefix up to the first cross-attention evaluated once for both '
                                'halves (rows are identical there); all three leave every output bit-identical'],
            'kernel_time_ms_est': {k: round(v['ms'] * a.profile_stride, 3) for k, v in prof.items()},
            'whole_path_tflops': value * tflop_per_image * (a.ddim_steps / DDIM_STEPS),
            'whole_path_mfma_frac': value * tflop_per_image * (a.ddim_steps / DDIM_STEPS) / (PEAK_TFLOPS * world),
            'executed_tflop_per_image': exec_tflop_per_image,
            'executed_tflops': value * exec_tflop_per_image * (a.ddim_steps / DDIM_STEPS),
            'executed_note': 'whole_path_* credit the reference\'s 107.2 TFLOP per image (SURVEY 8d); the CFG-pair prefix sharing '
                             'executes 4.08 GFLOP less per net, image and step with bit-identical outputs: executed_* is the '
                             'rate of the work actually run',
            'attention_tflops': (prof['attention']['work'] / (prof['attention']['ms'] * 1e-3) / 1e12
                                 if prof['attention']['ms'] > 0 else 0.0),
            'norm_GBps': (prof['norm']['work'] / (prof['norm']['ms'] * 1e-3) / 1e9 if prof['norm']['ms'] > 0 else 0.0),
            'first_stage_decode': None if dec_s is None else {
                'ms_per_image': dec_s / npg * 1e3, 'images_per_s_including_decode': N / (dt / a.steps + dec_s),
                'note': 'AutoencoderKL.decode of the sampled latents in the same engine, outside the timed region; '
                        '1.27 TFLOP/image'},
            'per_rank_images_per_s': per_rank,
            'twin_streams': os.environ.get('FGDM_TWIN_STREAMS') == '1',
            'full': a.full,
            'weights': {'params': n_params, 'load_s': round(load_s, 2), 'bcast_s': wt.get('bcast_s'),
                        'bcast_bytes': wt.get('bcast_bytes'),
                        'note': 'one broadcast of a flat buffer from rank 0 (RCCL over xGMI): fp16 for the tensors the engine '
                                'stores as fp16, fp32 for biases / norm affine / to_q; load_s includes generating the synthetic '
                                'weights on rank 0 and repacking on every rank'},
            'workspace': engine.workspace_stats(),
        }
        log(f'{value:.3f} images/s; igemm {achieved:.0f} TFLOP/s')
    if use_dist:            # the other ranks are done: release them before rank 0 spends its 20-30 s on the CPU baseline
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        if a.full and not a.no_cpu_baseline:
            res['cpu_baseline'] = cpu_baseline()       # rank 0's host cores, after the timed region, at every N
        emit(res)


if __name__ == '__main__':
    main()
