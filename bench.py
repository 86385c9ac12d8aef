#!/usr/bin/env python3
"""Headline benchmark: one training step of the I2-SDF render core on synthetic rays / random-weight networks.

    python bench.py [--gpus N] [--steps K] [--warmup W]

N > 1 without a torch.distributed environment: this script launches N ranks itself (torch.distributed.run on 127.0.0.1, one
rank per GPU, RCCL); under `python -m torch.distributed.run ... bench.py --gpus N` it is one of the ranks.  Rank 0 prints ONE
JSON line.

Workload (BASELINE.json configs[1]): synthetic.yml networks (8x256 SDF + 4x256 radiance MLP, 800 955 parameters,
reference init), 1024 rays per GPU, N_samples 64 -> 97 shaded samples per ray, camera (ii) of BASELINE.md (t=(0,0,-2),
beta=0.02, looking at the init sphere), sampler iteration count fixed to k=2 (it is data dependent).
A step = ray set-up -> error-bounded sampler (k SDF-MLP passes over 128 samples/ray) -> SDF MLP with d sdf/dx ->
radiance MLP -> density/compositing -> I2SDFLoss -> backward (double backward through the SDF MLP, all parameter
gradients) -> [N>1: one flat all-reduce] -> Adam step.  Inputs are resident in HBM before the timed region.
`value` = rays x 97 x N / step time (whole job, weak scaling: every rank draws its own 1024 rays).

Arithmetic: fp32 storage and fp32 accumulation everywhere; the matrix products run either on fp32-input MFMA or (default) as
bf16x3 split products on the bf16 MFMA pipe (three bf16 terms per fp32 operand, six partial products, error 2^-24:
fp32-equivalent, csrc/x3.h).  Since round 4 the 256x256 weight-gradient GEMMs use TWO bf16 terms per operand by default (three
products, per-product error <= 3 * 2^-18; every parameter gradient at 3e-6 of the fp64 oracle, the whole GPU suite runs in both
modes); the sub-record `wgrad_bf16x3` is the same step with the fp32-equivalent form there too -- `dtype` says which.

Timing: W warm-up steps, then --windows windows (default 1, so that the headline times exactly K steps) of EXACTLY K steps each, every
window bracketed by a barrier + device synchronisation on both sides and reduced with MAX over the ranks (sub-records: --sub-windows windows
each, median).  On one GPU `ms_per_step` / `value` are the MEDIAN timed step, read off HIP events recorded between the steps on the
caller's stream (a one-off stall moves one step, not the figure); with N ranks they are the MEDIAN window, max over the ranks (the
chip's DVFS and the boxes of the pool move a 20-step window by 1-2 %).  `windows_ms_per_step` lists the windows' wall times per step,
`ms_per_step_min` is the fastest.

--dump-outputs DIR: what the last timed headline step computed -- the render outputs, the loss terms, and after the optimizer step every
parameter gradient and parameter -- as DIR/<name>.npy (float32), at most 64 MB in all.  Weights (torch.manual_seed(0)), rays and ground
truth (seeded generators) are the same in every run with the same arguments, so two builds can be compared output for output.

Per-entry-point times (`kernels`, `roofline`): the timed steps run the per-point entry points as a CHAIN of point ranges on several
streams (include/i2sdf.h: I2SDF_OPT_PARTS), where an entry point has no duration of its own.  They are therefore measured live in
a second pass of --profile-steps steps right behind the timed windows, same process, same inputs, with every entry point joining its
ranges (HIP events on the stream the entry points are given, which then bracket all of an entry point's kernels).
`roofline.traffic`, `kernels_hbm` (HBM bytes and GB/s of the sampler / compositing kernels) and `kernels_mfma` (matrix-pipe occupancy of the
MLP kernels) come from three rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE, SQ counters: separate runs, counters only) that this script
starts itself on a 3-step run of the same workload.

Sub-records of the same JSON line: `dense128` (BASELINE.json's metric convention: 128 shaded samples/ray, sampler bypassed),
`strong` (fixed global batch of --strong-rays rays split over the ranks), `k1` / `k5` / `natural_k` (sampler iteration count fixed
to 1 / 5, and the data-dependent loop, instead of k=2), `wgrad_bf16x3` (fp32-equivalent arithmetic in the weight-gradient kernel too),
`rays4096` (BASELINE cfg 5: the per-GPU batch of the 8-GPU run), `cfg3` (synthetic_light_mask.yml networks), `cfg4_image` (one full
640x480 eval render through i2sdf_render_image), `allreduce_us` (the flat gradient all-reduce alone), `roofline`, `cpu_baseline` (the CPU restatement on this node's host cores: best thread count, 1 thread, all physical
cores), `eager_rocm_baseline` (the same restatement as stock PyTorch-ROCm eager ops on this GPU: the un-fused baseline of
BASELINE.md section 3).
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rays", type=int, default=1024, help="rays per GPU (weak-scaling headline)")
    ap.add_argument("--strong-rays", type=int, default=8192, help="global batch of the strong-scaling sub-record (split over the ranks)")
    ap.add_argument("--scaling", default="both", choices=["weak", "strong", "both"],
                    help="which scaling mode(s) to time; `value`/`scaling` of the JSON line are the weak ones unless --scaling strong")
    ap.add_argument("--sampler-iters", type=int, default=2, help="fixed sampler iterations k (0 = data dependent)")
    ap.add_argument("--windows", type=int, default=1, help="timed windows of --steps steps each (median reported); the default, one window, "
                                                           "makes --steps the number of timed steps of the headline")
    ap.add_argument("--sub-windows", type=int, default=3, help="timed windows of every sub-record (strong, dense128, k1, k5, natural_k, wgrad_bf16x3, rays4096, cfg3)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed headline step computed (render outputs, loss terms, parameter gradients, updated "
                         "parameters) as DIR/<name>.npy, float32, at most 64 MB in all (larger arrays as a fixed sample)")
    ap.add_argument("--profile-steps", type=int, default=10, help="steps of the per-entry-point timing pass behind the timed windows")
    ap.add_argument("--no-live-traffic", action="store_true", help="do not start the rocprofv3 --pmc passes for roofline.traffic / kernels_hbm")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)      # the run under rocprofv3: headline steps only, no output
    ap.add_argument("--cpu-probe", default="", help=argparse.SUPPRESS)               # "threads,rays,k,n_shaded": one bounded CPU measurement, prints JSON
    ap.add_argument("--selftest-launch", action="store_true",
                    help="launch-logic self-test WITHOUT a GPU: the same spawn / rendezvous / rank-0 JSON path with the render core replaced by the "
                         "CPU stand-in of tests/host_stub.py (needs --backend gloo for N>1); the line it prints is marked data=mock and carries no throughput claim")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the dense128 / natural_k / eager_rocm_baseline sub-records")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (nccl = RCCL; gloo only to smoke-test the N>1 path)")
    ap.add_argument("--dp-transport", default="auto", choices=["auto", "library", "torch"],
                    help="N>1: who carries the gradient all-reduce -- the library's own RCCL communicator (i2sdf_allreduce_grads; auto = this when the "
                         "backend is nccl, with fallback to torch if it cannot be created on every rank) or torch.distributed.all_reduce")
    ap.add_argument("--share-gpu", action="store_true", help="testing only: all ranks use cuda:0 (needs --backend gloo)")
    ap.add_argument("--equivalent", action="store_true",
                    help="N>1: 1-GPU-equivalent data parallelism (i2sdf_amd.dist.attach_data_parallel(equivalent=True) + attach_loss: the sampler's "
                         "convergence flag is MAX-reduced per iteration, rank 0's randperm columns are broadcast, the loss denominators are "
                         "averaged); throughput runs leave it off")
    ap.add_argument("--cpu-rays", type=int, default=512)
    ap.add_argument("--fused-adam", type=int, default=1, help="1: i2sdf_amd.FusedAdam (one HIP launch over the flat buffer); 0: torch.optim.Adam")
    ap.add_argument("--bf16x3", type=int, default=-1,
                    help="bit mask of the kernels that run in bf16x3 split arithmetic (1 sampler forward, 2 weight gradients, "
                         "4 training forward, 8 SDF backward, 16 radiance net); -1 = the engine's default (all available), 0 = plain fp32 MFMA everywhere")
    return ap.parse_args()


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn(args):
    """--gpus N with no torch.distributed environment: become the launcher (one rank per GPU, rendezvous on 127.0.0.1)."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def flops_per_point(cfg):
    """Algorithmic dense-contraction FLOPs (2 x MACs) per point for each kernel family."""
    sdf, rgb = cfg.sdf.dims, cfg.rgb.dims
    F = cfg.feature_size
    mac_fwd_hidden = sum(o * i for o, i in sdf[:-1])
    mac_fwd = mac_fwd_hidden + sdf[-1][0] * sdf[-1][1]
    mac_igrad = mac_fwd_hidden + sdf[-1][1]                      # reverse chain; last layer contributes row 0 only
    mac_rgb = sum(o * i for o, i in rgb)
    return {
        "sdf_forward": 2 * (mac_fwd_hidden + sdf[-1][1]),          # sampler: sdf row only
        "sdf_forward_grad": 2 * (mac_fwd + mac_igrad),
        "rgb_forward": 2 * mac_rgb,
        "rgb_backward": 2 * (mac_rgb - rgb[0][0] * (rgb[0][1] - F)),   # input grad for the feature columns only
        "sdf_backward": 2 * (mac_igrad + mac_fwd - sdf[0][0] * sdf[0][1]),
        "wgrad_sdf": 2 * (mac_igrad + mac_fwd),
        "wgrad_rgb": 2 * mac_rgb,
    }


def bytes_per_point(cfg):
    """HBM bytes per point of the saved-tensor traffic THIS DESIGN moves, fp32 (DESIGN.md "Data layout"): every tensor counted
    once per kernel that reads or writes it.  It is the design's own traffic, not a compulsory minimum: the compulsory I/O of these
    kernels is ~1 KB/point (the MLP kernels are MFMA-bound)."""
    H, F = cfg.sdf.hidden, cfg.feature_size
    nh = cfg.sdf.n_lin - 1                         # hidden activations h_1..h_{L-1} of the SDF net
    nr = cfg.rgb.n_lin - 1
    row, frow = 4 * H, 4 * F
    return {
        "i2sdf_sdf_forward_grad": nh * row * 3 + frow + 160 + 28,      # write h, write abar, re-read h (chain), feature, PE, sdf/grad
        "i2sdf_sdf_backward": nh * row * (2 + 4) + frow + 200,  # sweep 1: read h, write G(hbar); sweep 2: read h, abar, G(hbar), write G(a) (round 5: G2 formed in sweep 2)
        "i2sdf_weight_grads": nh * row * 4 + row + frow + nr * 2 * 4 * cfg.rgb.hidden + frow + 288,   # A, A', B, B' per SDF layer; rgb G(a), r
        "i2sdf_rgb_forward": frow + nr * 4 * cfg.rgb.hidden + 128 + 12,
        "i2sdf_rgb_backward": nr * 4 * cfg.rgb.hidden * 2 + frow + 40,
    }


class Workload:
    """One rank's training-step workload: `rays` rays of the synthetic camera, the synthetic.yml networks, loss, optimizer."""

    def __init__(self, args, dev, rank, world, light=False):
        import torch
        from i2sdf_amd import I2SDFNetwork, I2SDFLoss, synthetic_conf
        from i2sdf_amd import dist as i2dist
        self.torch, self.dev, self.rank, self.world, self.args = torch, dev, rank, world, args
        conf = synthetic_conf(light)               # light: synthetic_light_mask.yml (adds the light-mask head; BASELINE cfg 3)
        conf["use_normal"] = True
        torch.manual_seed(0)                                  # identical initial weights on every rank
        self.net = I2SDFNetwork(conf).to(dev)
        with torch.no_grad():
            self.net.density.beta.fill_(0.02)
        self.net.train()
        self.loss_fn = I2SDFLoss(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=150000, depth_weight=0.1, normal_weight=0.05,
                                 light_mask_weight=0.5 if light else 0.0)   # synthetic.yml:15-23 / synthetic_light_mask.yml
        if args.fused_adam:
            from i2sdf_amd import FusedAdam
            self.opt = FusedAdam(self.net, lr=5.0e-4, eps=1e-15)         # model/trainer/recon.py:203 (Adam, lr 5e-4)
        else:
            self.opt = torch.optim.Adam(self.net.get_param_groups(5.0e-4), eps=1e-15)
        if world > 1:
            i2dist.attach_data_parallel(self.net, native={"auto": None, "library": True, "torch": False}[args.dp_transport],
                                        equivalent=bool(getattr(args, "equivalent", False)))
            if getattr(args, "equivalent", False):
                i2dist.attach_loss(self.loss_fn, self.net)
        self.step_no = 0

    def inputs(self, B, seed):
        torch, dev = self.torch, self.dev
        g = torch.Generator().manual_seed(seed)
        W_, H_ = 640, 480
        K = torch.eye(4); K[0, 0] = K[1, 1] = 600.0; K[0, 2] = W_ / 2; K[1, 2] = H_ / 2
        pose = torch.eye(4); pose[:3, 3] = torch.tensor([0.0, 0.0, -2.0])
        uv = torch.stack([torch.randint(0, W_, (B,), generator=g), torch.randint(0, H_, (B,), generator=g)], -1).float().reshape(B, 1, 2)
        inp = {"uv": uv.to(dev), "intrinsics": K.repeat(B, 1, 1).to(dev), "pose": pose.repeat(B, 1, 1).to(dev)}
        gt = {"rgb": torch.rand(B, 3, generator=g).to(dev), "depth": (torch.rand(B, generator=g) * 3).to(dev),
              "depth_mask": torch.ones(B, dtype=torch.bool, device=dev),
              "normal": torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).to(dev),
              "normal_mask": torch.ones(B, dtype=torch.bool, device=dev),
              "light_mask": (torch.rand(B, 1, generator=g) > 0.5).float().to(dev)}
        return inp, gt

    def fence(self):
        if self.world > 1:
            self.torch.distributed.barrier()
        self.torch.cuda.synchronize()

    def run(self, B, seed, k_iters, steps, warmup, dense=0, timing=False, windows=1, profile_steps=0, no_sync=False, keep_last=False):
        """-> dict(dt = median over `windows` windows of the seconds for `steps` steps (each max over ranks), dts, loss, iters, ktimes).
        dense > 0: `dense` uniform samples per ray, sampler bypassed (the dense-128 convention).
        no_sync: the same steps with the gradient all-reduce suspended (i2sdf_amd.dist.no_sync) -- what the collective costs a step.
        keep_last: also return `last`, host copies of what the last timed step handed its caller (see last_step_arrays)."""
        torch, net = self.torch, self.net
        import contextlib
        from i2sdf_amd import dist as i2dist
        sync_ctx = (lambda: i2dist.no_sync(net)) if no_sync else contextlib.nullcontext
        inp, gt = self.inputs(B, seed)
        net.force_iters = k_iters
        zs = None
        if dense:
            eng = net._engine_for(self.dev)
            c, d, nrm = eng.ray_setup(inp["uv"], inp["pose"], inp["intrinsics"])
            z = torch.linspace(0.0, 6.0, dense + 1, device=self.dev).repeat(B, 1).contiguous()      # n samples + z_max column
            zs = (c, d, nrm, z, z[:, dense // 2:dense // 2 + 1].contiguous())
        kept = {}

        def step(keep=False):
            with sync_ctx():
                out = net.render(inp, *zs) if zs else net(inp)
                losses = self.loss_fn(out, gt, self.step_no)
                self.opt.zero_grad(set_to_none=True)
                losses["loss"].backward()
            self.opt.step()
            self.step_no += 1
            if keep:
                kept["out"], kept["losses"] = out, losses
            return losses["loss"]

        for _ in range(max(warmup, 1)):
            step()
        eng = net._engine_for(self.dev)
        dts = []
        n_win = max(windows, 1)
        # one GPU: an event on the caller's stream behind every timed step, so that a step's time can be read off the device timeline
        # (the median step of the headline shrugs off a one-off stall that would move a single window's wall time)
        evs = [[torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)] for _ in range(n_win)] if (timing and self.world == 1 and self.dev.type == "cuda") else None
        for w in range(n_win):                                 # every window: exactly `steps` steps, barrier + synchronize on both sides
            self.fence()
            t0 = time.perf_counter()
            if evs:
                evs[w][0].record()
            for s in range(steps):
                loss = step(keep_last and w == n_win - 1 and s == steps - 1)
                if evs:
                    evs[w][s + 1].record()
            self.fence()
            dts.append(time.perf_counter() - t0)
        step_ms = sorted(a.elapsed_time(b) for e in evs for a, b in zip(e[:-1], e[1:])) if evs else None
        last = self.last_step_arrays(kept["out"], kept["losses"]) if kept else None
        t = torch.tensor(dts, dtype=torch.float64, device=self.dev)
        dts_min = None
        if self.world > 1:
            tmin = t.clone()
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            torch.distributed.all_reduce(tmin, op=torch.distributed.ReduceOp.MIN)      # the fastest rank's view of the same windows: a straggler shows as a spread
            dts_min = [float(x) for x in tmin.tolist()]
        dts = [float(x) for x in t.tolist()]
        ktimes, prof_steps = None, 0
        if timing and profile_steps > 0:
            # per-entry-point pass: every entry point joins its point ranges, so the events on the caller's stream bracket all its kernels
            eng.use_chain = False
            step()
            self.fence()
            eng.start_timing()
            for _ in range(profile_steps):
                step()
            self.fence()
            ktimes, prof_steps = eng.stop_timing(), profile_steps
            eng.use_chain = True
        med = sorted(dts)[len(dts) // 2]
        return {"dt": med, "dts": dts, "dts_rank_min": dts_min, "loss": float(loss.item()), "iters": int(net.last_sampler_iters.item()) if not dense else 0,
                "ktimes": ktimes, "prof_steps": prof_steps, "eng": eng, "last": last, "step_ms": step_ms}

    def last_step_arrays(self, out, losses):
        """name -> host float array of what one training step hands its caller: the render outputs (out.*), the loss terms (loss.*),
        and after the optimizer step every parameter gradient (grad.*) and updated parameter (param.*)."""
        torch = self.torch

        def host(x):
            return x.detach().float().cpu().numpy()
        arrs = {}
        for k, v in out.items():
            if torch.is_tensor(v):
                arrs["out." + k] = host(v)
        for k, v in losses.items():
            if torch.is_tensor(v):
                arrs["loss." + k] = host(v)
        for n, p in self.net.named_parameters():
            if p.grad is not None:
                arrs["grad." + n] = host(p.grad)
            arrs["param." + n] = host(p)
        return arrs


DUMP_LIMIT = 64 * 2 ** 20          # bytes, all --dump-outputs files together


def dump_outputs(arrs, path, limit=DUMP_LIMIT):
    """--dump-outputs: one DIR/<name>.npy per array.  If they exceed `limit` together, every array larger than an equal share of
    what the whole ones leave is replaced by a fixed sample of its flattened elements (seeded by the array's name: the same
    positions in every run with the same arguments)."""
    import zlib
    import numpy as np
    os.makedirs(path, exist_ok=True)
    sizes = sorted((a.nbytes, k) for k, a in arrs.items())
    left = share = limit - 256 * len(arrs)          # (room for the .npy headers)
    for i, (nb, k) in enumerate(sizes):            # smallest first: the share of the remaining ones only grows
        share = left // (len(sizes) - i)
        if nb > share:
            break
        left -= nb
    for k, a in arrs.items():
        a = np.ascontiguousarray(a)
        if a.nbytes > share:
            m = max(share // a.itemsize, 1)
            idx = np.random.default_rng(zlib.crc32(k.encode())).choice(a.size, size=m, replace=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(path, k + ".npy"), a)


class _MockEngine:
    """what main() reads off the engine, for --selftest-launch"""
    n_z, parts, use_chain = 98, 0, True
    sdf_forward_bf16x3 = train_forward_bf16x3 = sdf_backward_bf16x3 = wgrad_bf16x3 = wgrad_bf16x2 = rgb_bf16x3 = sampler_bf16x2 = False

    def start_timing(self):
        pass

    def stop_timing(self):
        return {}


class MockWorkload(Workload):
    """--selftest-launch: the real module wiring (flat parameter buffer, grad_sync hook, attach_data_parallel) over the CPU stand-in core
    of tests/host_stub.py; no GPU, no kernels -- it exists so that the N>1 launch path can be exercised on a CPU box."""

    def __init__(self, args, dev, rank, world):
        import torch
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from host_stub import HostStubNetwork
        from i2sdf_amd import synthetic_conf
        from i2sdf_amd import dist as i2dist
        self.torch, self.dev, self.rank, self.world, self.args = torch, dev, rank, world, args
        torch.manual_seed(0)
        self.net = HostStubNetwork(synthetic_conf())
        self.net._ensure_flat()
        self.opt = torch.optim.SGD(self.net.parameters(), lr=1e-3)
        self.xchg_calls = 0
        if world > 1:
            i2dist.attach_data_parallel(self.net, equivalent=bool(getattr(args, "equivalent", False)))
        self.step_no = 0
        self.eng = _MockEngine()
        self.net.last_sampler_iters = torch.tensor([args.sampler_iters or 5])
        self.net._engine_for = lambda dev_: self.eng

    def loss_fn(self, out, gt, step):
        st = getattr(self.net, "dp_state", None)
        if st is not None and st.equivalent and st.enabled:
            # `equivalent` mode without kernels: the exchanges the device-side hooks of a real step issue, in their order and count, through
            # the same TorchExchange object and process group -- one MAX of the sampler's 4-byte convergence flag per enqueued sampler
            # iteration (sampler.hip), then one AVG of the loss denominators (loss.hip) -- so that a rank that issued a different sequence
            # would hang or mis-reduce HERE, on the CPU box, and not in the first N-GPU run
            from i2sdf_amd import lib as L_
            torch = self.torch
            for it in range(5):                                   # max_total_iters iterations are always enqueued
                flag = torch.tensor([1 if (self.rank + it + self.step_no) % self.world == 0 else 0], dtype=torch.int32)
                st.xchg.reduce_(flag, L_.XCHG_MAX)
                assert int(flag.item()) == 1, "MAX over the ranks: exactly one rank raised the flag in this iteration"
            cnt = torch.tensor([64.0, 0.0, float(10 + self.rank), float(20 + 2 * self.rank)])
            st.xchg.reduce_(cnt, L_.XCHG_AVG)
            w = self.world
            assert abs(float(cnt[2]) - (10 + (w - 1) / 2.0)) < 1e-5 and abs(float(cnt[3]) - (20 + (w - 1))) < 1e-5, cnt
            self.xchg_calls = st.xchg.calls
        return {"loss": ((out["rgb_values"] - gt["rgb"]) ** 2).mean()}

    def fence(self):
        if self.world > 1:
            self.torch.distributed.barrier()

    def run(self, B, seed, k_iters, steps, warmup, dense=0, timing=False, windows=1, profile_steps=0, no_sync=False, keep_last=False):
        self.args_dense = dense
        return Workload.run(self, min(B, 64), seed, k_iters, steps, warmup, dense=0, timing=timing, windows=windows, profile_steps=0, no_sync=no_sync,
                            keep_last=keep_last)


def main():
    args = parse()
    if args.cpu_probe:
        return cpu_probe(args.cpu_probe)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn(args))
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    mock = args.selftest_launch
    assert mock or torch.cuda.is_available(), "bench.py needs an MI355X"
    if mock and world > 1 and args.backend != "gloo":
        raise SystemExit("bench.py --selftest-launch runs on the CPU: use --backend gloo")
    if not mock and world > 1 and not args.share_gpu and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: {world} ranks requested but only {torch.cuda.device_count()} GPU(s) visible "
                         "(--share-gpu --backend gloo runs all ranks on cuda:0 to smoke-test the N>1 path)")
    dev_index = 0 if (world == 1 or args.share_gpu) else local_rank
    if not mock:
        torch.cuda.set_device(dev_index)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(args.backend)
    dev = torch.device("cpu") if mock else torch.device("cuda", dev_index)

    wl = (MockWorkload if mock else Workload)(args, dev, rank, world)
    if mock:
        args.no_extras = args.no_cpu_baseline = args.no_live_traffic = True
    B = args.rays
    wl.run(B, 1000 + rank, args.sampler_iters, 1, 1)        # builds the engine (and the flat parameter buffer) the way a trainer would
    eng = wl.net._engine_for(dev)
    if args.bf16x3 >= 0:
        eng.set_sdf_forward_bf16x3(bool(args.bf16x3 & 1))
        eng.set_wgrad_bf16x3(bool(args.bf16x3 & 2))
        eng.set_train_forward_bf16x3(bool(args.bf16x3 & 4))
        eng.set_sdf_backward_bf16x3(bool(args.bf16x3 & 8))
        eng.set_rgb_bf16x3(bool(args.bf16x3 & 16))
    n_shaded = eng.n_z - 1
    K, W = args.steps, args.warmup
    if args.pmc_child:            # under rocprofv3 --pmc (live_traffic below): the headline steps only, nothing to report
        wl.run(B, 1000 + rank, args.sampler_iters, K, W)
        return

    # ---- headline: weak scaling, every rank draws its own `rays` rays -----------------------------------------------
    SW = max(args.sub_windows, 1)
    weak = strong = None
    dump = args.dump_outputs is not None and rank == 0
    if args.scaling in ("weak", "both"):
        weak = wl.run(B, 1000 + rank, args.sampler_iters, K, W, timing=True, windows=args.windows,
                      profile_steps=args.profile_steps, keep_last=dump)      # each rank draws its own rays (ray-sharded data parallelism)
    if args.scaling in ("strong", "both"):
        Bs = args.strong_rays // world                    # fixed GLOBAL batch, split over the ranks
        strong = wl.run(Bs, 2000 + rank, args.sampler_iters, K, W, timing=(weak is None), windows=(args.windows if weak is None else SW),
                        profile_steps=(args.profile_steps if weak is None else 0), keep_last=(dump and weak is None))
        strong["rays_per_gpu"] = Bs
    head = weak if weak is not None else strong
    if dump:
        dump_outputs(head.pop("last"), args.dump_outputs)
    head_B = B if weak is not None else strong["rays_per_gpu"]
    dt, iters, ktimes = head["dt"], head["iters"], head["ktimes"]
    if head["step_ms"]:             # one GPU: the median timed step on the device timeline (HIP events between the steps)
        dt = head["step_ms"][len(head["step_ms"]) // 2] * 1e-3 * K
    ms = dt / K * 1e3
    value = head_B * n_shaded * world / (dt / K)

    def sub(r, rays, shaded, workload, **more):
        """a sub-record from a Workload.run() result: median of its windows, the windows themselves, us per ray"""
        d = {"value": round(rays * shaded * world / (r["dt"] / K), 1), "unit": "ray-samples/s", "ms_per_step": round(r["dt"] / K * 1e3, 4),
             "windows_ms_per_step": [round(x / K * 1e3, 4) for x in r["dts"]], "us_per_ray": round(r["dt"] / K / rays * 1e6, 4), "workload": workload}
        d.update(more)
        return d

    extras = {}
    if not args.no_extras:
        d128 = wl.run(B, 1000 + rank, 0, K, W, dense=128, windows=SW)
        extras["dense128"] = sub(d128, B, 128, f"{B} rays/GPU x 128 uniform shaded samples, sampler bypassed (BASELINE.json metric convention), same step otherwise")
        # the fp32-equivalent form of the ONE kernel family that runs narrower by default: the 256x256 weight-gradient blocks with three
        # bf16 planes per operand and six products instead of two and three (I2SDF_OPT_WGRAD_BF16X2 off); everything else unchanged
        sx2 = bool(getattr(eng, "sampler_bf16x2", False))
        if eng.wgrad_bf16x3 and eng.wgrad_bf16x2:
            eng.set_wgrad_bf16x2(False)
            if sx2:
                eng.set_sampler_bf16x2(False)
            x3r = wl.run(B, 1000 + rank, args.sampler_iters, K, W, windows=SW)
            eng.set_wgrad_bf16x2(True)
            if sx2:
                eng.set_sampler_bf16x2(True)
            extras["wgrad_bf16x3"] = sub(x3r, B, n_shaded, "the headline step with the weight-gradient GEMMs AND the sampler's sdf-only passes in bf16x3 too "
                                         "(I2SDF_OPT_WGRAD_BF16X2 and I2SDF_OPT_SAMPLER_BF16X2 off: three bf16 terms per operand, six products): fp32-equivalent "
                                         "arithmetic in EVERY kernel of the step -- the round-3 headline convention")
        if getattr(eng, "saves24", False) and eng.wgrad_bf16x2:
            # abars / G(hbar) / G(a) in fp32 storage, everything else as in the headline: what I2SDF_OPT_SAVES24 buys (round 6)
            eng.set_saves24(False)
            extras["saves_fp32"] = sub(wl.run(B, 1000 + rank, args.sampler_iters, K, W, windows=SW), B, n_shaded,
                                       "headline step with abars / G(hbar) / G(a) of the SDF net stored as fp32 (I2SDF_OPT_SAVES24 off), everything else unchanged")
            eng.set_saves24(True)
        if sx2:
            # the sampler's passes in the fp32-equivalent form, everything else as in the headline: what I2SDF_OPT_SAMPLER_BF16X2 buys (round 6)
            eng.set_sampler_bf16x2(False)
            s3 = {"k%d" % args.sampler_iters: sub(wl.run(B, 1000 + rank, args.sampler_iters, K, W, windows=SW), B, n_shaded, "headline step, sampler passes with three bf16 planes"),
                  "natural_k": sub(wl.run(B, 1000 + rank, 0, K, W, windows=SW), B, n_shaded, "data-dependent sampler loop, sampler passes with three bf16 planes")}
            if world == 1 and not mock:
                s3["cfg4_image"] = full_image(wl, dev, n_shaded)
            eng.set_sampler_bf16x2(True)
            extras["sampler_bf16x3"] = s3
        for kk in (1, 5):
            if kk != args.sampler_iters:
                extras[f"k{kk}"] = sub(wl.run(B, 1000 + rank, kk, K, W, windows=SW), B, n_shaded,
                                       f"same as the headline with the sampler iteration count fixed to k={kk}")
        nat = wl.run(B, 1000 + rank, 0, K, W, windows=SW)
        extras["natural_k"] = sub(nat, B, n_shaded, "same as the headline with the data-dependent sampler loop (all max_total_iters iterations enqueued, device flag)",
                                  sampler_iters_observed=nat["iters"])
        # BASELINE.json configs[4]: the per-GPU batch of the 8-GPU run (4096 rays per GPU), here on this rank's GPU
        if B != 4096:
            extras["rays4096"] = sub(wl.run(4096, 3000 + rank, args.sampler_iters, K, W, windows=SW), 4096, n_shaded,
                                     "BASELINE cfg 5 per-GPU batch: 4096 rays/GPU, same nets / camera / k, training step incl. loss, backward, optimizer")
        if world == 1 and not mock:
            # BASELINE.json configs[2]: synthetic_light_mask.yml networks (adds the light-mask head and its loss term)
            wl3 = Workload(args, dev, rank, world, light=True)
            r3 = wl3.run(B, 1000 + rank, args.sampler_iters, K, W, windows=SW)
            extras["cfg3"] = sub(r3, B, n_shaded, "BASELINE cfg 3: synthetic_light_mask.yml nets (8x256 SDF + 4x256 radiance + light-mask head), "
                                                  f"{B} rays, k={args.sampler_iters}, training step incl. loss (light_mask_weight 0.5), backward, optimizer")
            del wl3, r3
            extras["cfg4_image"] = full_image(wl, dev, n_shaded)
        extras["allreduce_us"] = allreduce_alone(wl, dev, world)
    elif mock and world > 1:
        extras["allreduce_us"] = allreduce_alone(wl, dev, world)      # the launch self-test exercises the record the first N-GPU run will carry
    if world > 1 and weak is not None and not getattr(args, "equivalent", False):
        # (not in --equivalent mode: there the sampler's flag exchange keeps running under no_sync(), the pair would not isolate the all-reduce)
        # what the one collective of a step costs THE STEP (not the collective timed alone): the headline step once more with the gradient
        # all-reduce suspended (i2sdf_amd.dist.no_sync); exposed = headline - that.  The ranks' weights drift apart meanwhile (every rank
        # applies its own gradient): rank 0's parameters are broadcast again afterwards.  Last of the timed runs on purpose.
        from i2sdf_amd import dist as i2dist
        ns = wl.run(B, 1000 + rank, args.sampler_iters, K, W, windows=SW, no_sync=True)
        i2dist.broadcast_parameters(wl.net)
        extras["step_ms_without_allreduce"] = round(ns["dt"] / K * 1e3, 4)
        extras["exposed_allreduce_ms"] = round((weak["dt"] - ns["dt"]) / K * 1e3, 4)
        extras["exposed_allreduce_note"] = ("ms_per_step minus the same step under no_sync() (median of %d windows each, max over ranks); next to "
                                            "allreduce_us (the collective alone) it says how much of the collective the step does not hide" % SW)
    if world > 1 and getattr(args, "equivalent", False):
        st_ = getattr(wl.net, "dp_state", None)
        xc = getattr(st_, "xchg", None)
        extras["equivalent"] = {"on": bool(st_ is not None and st_.equivalent),
                                "exchange_calls": int(getattr(xc, "calls", 0)) if xc is not None and hasattr(xc, "calls") else None,
                                "note": "1-GPU-equivalent mode: MAX of the sampler flag per iteration + AVG of the loss denominators per step through the exchange hook"}

    result = None
    live = live_traffic(args) if (rank == 0 and world == 1) else None
    if rank == 0:
        cfg = wl.net.cfg
        fp = flops_per_point(cfg)
        M_main, M_sdf = head_B * n_shaded, head_B * n_shaded + 3 * head_B
        launch_flops = {
            # the sampler entry point = k SDF-MLP passes over 128 samples/ray + the per-ray Algorithm-1 kernels (counted as 0 FLOP)
            "i2sdf_sample_rays": fp["sdf_forward"] * head_B * cfg.sampler.N_samples_eval * max(iters, 1),
            "i2sdf_sdf_forward_grad": fp["sdf_forward_grad"] * M_sdf,
            "i2sdf_rgb_forward": fp["rgb_forward"] * M_main,
            "i2sdf_rgb_backward": fp["rgb_backward"] * M_main,
            "i2sdf_sdf_backward": fp["sdf_backward"] * M_sdf,
            "i2sdf_weight_grads": fp["wgrad_sdf"] * M_sdf + fp["wgrad_rgb"] * M_main,
        }
        kern = {}
        KP = max(head["prof_steps"], 1)
        for name, (tot_ms, cnt) in (ktimes or {}).items():
            kern[name] = {"ms_per_step": tot_ms / KP, "launches_per_step": cnt / KP}
            if name in launch_flops and cnt:
                kern[name]["tflops"] = launch_flops[name] / (tot_ms / cnt * 1e-3) / 1e12
        mfma_names = [n for n in kern if "tflops" in kern[n]]
        dom = max(mfma_names, key=lambda n: kern[n]["ms_per_step"]) if mfma_names else None    # dominant = largest share of the step
        PEAK = 157.3            # TFLOP/s, fp32-input MFMA on MI355X (MI355X_MICROARCH.md)
        PEAK_BF16 = 2500.0      # TFLOP/s dense bf16 MFMA
        PEAK_X3 = PEAK_BF16 / 6  # six bf16 MFMAs per fp32 product block (csrc/x3.h): fp32-equivalent TFLOP/s at 100 % bf16 issue
        x3 = {"i2sdf_sample_rays": eng.sdf_forward_bf16x3, "i2sdf_sdf_forward_grad": eng.train_forward_bf16x3,
              "i2sdf_sdf_backward": eng.sdf_backward_bf16x3, "i2sdf_weight_grads": eng.wgrad_bf16x3,
              "i2sdf_rgb_forward": eng.rgb_bf16x3, "i2sdf_rgb_backward": eng.rgb_bf16x3}
        # the roof of an entry point: six bf16 MFMAs per fp32 product block (bf16x3), fp32-input MFMA otherwise; the weight-gradient GEMMs
        # with two bf16 terms per operand issue THREE MFMAs per product block: their roof is twice as high, and their fraction is priced against it
        def peak_of(n):
            if n == "i2sdf_weight_grads" and eng.wgrad_bf16x3 and eng.wgrad_bf16x2:
                return PEAK_BF16 / 3
            if n == "i2sdf_sample_rays" and eng.sdf_forward_bf16x3 and getattr(eng, "sampler_bf16x2", False):
                return PEAK_BF16 / 3      # two planes per operand, three products per block
            return PEAK_X3 if x3.get(n) else PEAK
        roof = None
        if dom:
            # the MLP kernels are dense contractions at ~1e6 FLOP per 12-byte point -> the roof is the MFMA peak of
            # the datatype used.  achieved = algorithmic FLOPs (fp32 products, SURVEY per-point figures x points) / mean duration.
            ach = kern[dom]["tflops"]
            peak = peak_of(dom)
            npts = {"i2sdf_rgb_forward": M_main, "i2sdf_rgb_backward": M_main}.get(dom, M_sdf)
            design_bytes = bytes_per_point(cfg).get(dom, 0) * npts
            t_launch = kern[dom]["ms_per_step"] / max(kern[dom]["launches_per_step"], 1e-9) * 1e-3
            traffic = entry_traffic(live, dom)
            src = "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes started by this run (2 x FETCH + WRITE, all kernels of the entry point, per step)"
            if traffic is None:
                traffic, src = profiled_traffic(dom)
            roof = {"bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                    "kernel": dom, "arithmetic": "bf16x3 split (fp32-equivalent FLOPs; peak = 2500 TFLOP/s dense bf16 / 6 MFMAs per product block)"
                    if x3.get(dom) else "f32 MFMA",
                    "bf16_mfma_issue_tflops": round(ach * 6, 1) if x3.get(dom) else None,
                    "algorithmic_flops": int(launch_flops[dom]), "launch_ms": round(t_launch * 1e3, 4),
                    "traffic": traffic, "traffic_source": src,
                    # the design's own saved-tensor traffic (NOT compulsory: recomputation / fusion would remove it) against HBM peak
                    "hbm_view": {"design_bytes": int(design_bytes), "gbs": round(design_bytes / t_launch / 1e9, 1), "peak_gbs": 8000.0,
                                 "frac": round(design_bytes / t_launch / 8.0e12, 4)},
                    "frac_vs_fp32_mfma_peak": round(ach / PEAK, 4),
                    # every MFMA-bound entry point against the same kind of peak (the dominant one above is simply the longest of them)
                    "entry_points": {n: {"ms": round(kern[n]["ms_per_step"], 4), "tflops": round(kern[n]["tflops"], 2),
                                         "frac": round(kern[n]["tflops"] / peak_of(n), 4)} for n in mfma_names},
                    # what the power limit leaves of the nominal peak: a pure v_mfma_f32_32x32x16_bf16 loop on random operands holds
                    # 1.95 GHz at 95 % matrix-pipe occupancy on this chip = 1933 TFLOP/s (scripts/ubench, profiles/r3_ubench_mfma_stage.txt)
                    "power_limited_bf16_peak_measured": {"tflops": 1933.0, "frac_of_nominal": 0.773,
                                                         "frac_of_it": round(ach * 6 / 1933.0, 4) if x3.get(dom) else None},
                    "all_mfma_kernels_tflops": round(sum(launch_flops[n] * kern[n]["launches_per_step"] for n in mfma_names)
                                                     / (sum(kern[n]["ms_per_step"] for n in mfma_names) * 1e-3) / 1e12, 2)}
        if roof is not None and live:
            roof["dominant_kernel"] = dominant_kernel(live, cfg, fp, eng, head_B, M_main, M_sdf, max(iters, 1), PEAK, PEAK_BF16)
        total_flops = sum(launch_flops.values())
        any_x3 = any(x3.values())
        result = {
            "metric": "ray-samples/sec (fwd+bwd)", "value": round(value, 1), "unit": "ray-samples/s", "n_gpus": world, "steps": K,
            "warmup": W, "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak" if weak is not None else "strong",
            "windows_ms_per_step": [round(x / K * 1e3, 4) for x in head["dts"]], "ms_per_step_min": round(min(head["dts"]) / K * 1e3, 4),
            "timing": (f"{len(head['dts'])} window(s) of exactly {K} steps each (barrier + synchronize around every window); ms_per_step: the median "
                       f"of the {len(head['step_ms'])} timed steps, HIP events between the steps" if head["step_ms"] else
                       f"median of {len(head['dts'])} windows of exactly {K} steps each (barrier + synchronize around every window, max over ranks)"),
            "vs_baseline": None,
            "dtype": "f32" if not any_x3 else ("f32 (bf16x3 split MFMA: fp32 operands as 3 bf16 terms, fp32 accumulate"
                                                + ("; the 256x256 weight-gradient GEMM blocks" + (" and the sampler's depth-choosing sdf-only passes" if getattr(eng, "sampler_bf16x2", False) else "")
                                                   + ": 2 bf16 terms per operand, 3 products, fp32 accumulate"
                                                   + ("; the saved SDF tensors abar / G(hbar) / G(a) -- operands of those GEMMs and of the second-order injection -- stored with 16 "
                                                      "significant bits in 3 bytes per value (saves_fp32: the same step with fp32 storage)" if getattr(eng, "saves24", False) else "")
                                                   + " -- see wgrad_bf16x3 for the all-fp32-equivalent step)"
                                                   if eng.wgrad_bf16x2 else ")")),
            "data": "synthetic" if not mock else "mock (launch-logic self-test on the CPU stand-in core: value / ms_per_step carry NO throughput claim)",
            "config": {"workload": "synthetic.yml nets (8x256 SDF + 4x256 radiance, 800955 params), training step incl. sampler, loss, backward, Adam",
                       "rays_per_gpu": head_B, "shaded_samples_per_ray": n_shaded, "sampler_iters": iters, "sampler_samples_per_iter": cfg.sampler.N_samples_eval,
                       "camera": "t=(0,0,-2), R=I, f=600, beta=0.02", "parallelism": f"dp{world} (ray-sharded, 1 flat grad all-reduce" + (
                           "" if world == 1 else (": library RCCL communicator, i2sdf_allreduce_grads" if getattr(wl.net.dp_state, "comm", None) is not None
                                                  else ": torch.distributed all_reduce")) + ")",
                       "optimizer": "i2sdf_amd.FusedAdam (1 launch)" if args.fused_adam else "torch.optim.Adam",
                       "backend": (args.backend if world > 1 else None), "world_size_observed": (dist.get_world_size() if world > 1 else 1),
                       "equivalent": bool(world > 1 and getattr(args, "equivalent", False))},
            "rays_per_s": round(head_B * world / (dt / K), 1),
            "step_tflops": round(total_flops * world / (dt / K) / 1e12, 2),
            # time the step's FLOPs need at each entry point's own MFMA roof (bf16x3: 2500/6, bf16x2 weight gradients: 2500/3, fp32: 157.3
            # TFLOP/s) over the measured step time, per GPU
            "frac_bf16x3_mfma_roofline_whole_step": round(sum(launch_flops[n] / (peak_of(n) * 1e12) for n in launch_flops) / (dt / K), 4) if any_x3 else None,
            "frac_fp32_mfma_roofline_whole_step": round(total_flops / (dt / K) / 1e12 / PEAK, 4),   # per GPU (weak scaling)
            "final_loss": head["loss"],
            "roofline": roof, "kernels": {k: {kk: round(vv, 4) for kk, vv in v.items()} for k, v in kern.items()},
            "kernels_note": f"per-entry-point HIP-event times of a {head['prof_steps']}-step pass behind the timed windows in which every entry point joins its point "
                            f"ranges (parts = {eng.parts}); in the timed steps the ranges of consecutive entry points overlap, so these do not add up to ms_per_step",
        }
        if live:
            # the per-ray kernels (sampler non-MLP part, compositing) are priced against HBM bandwidth: bytes moved and GB/s
            # per launch from the PMC passes (kernels serialised there, so `us` is the kernel running alone)
            hb = {}
            for k, v in live.items():
                short = _short(k)
                if any(q in short for q in ("composite_", "sampler_", "beta_reduce", "raygen", "loss_", "draws_")) and v.get("us", 0) > 0:
                    e = hb.setdefault(short, {"bytes": 0.0, "us": 0.0, "launches_per_step": 0.0})
                    e["bytes"] += (v["fetch"] + v["write"]) * v["n"]; e["us"] += v["us"] * v["n"]; e["launches_per_step"] += v["n"]
            result["kernels_hbm"] = {k: {"bytes_per_launch": round(e["bytes"] / e["launches_per_step"]), "us_per_launch": round(e["us"] / e["launches_per_step"], 2),
                                         "gbs": round(e["bytes"] / e["us"] / 1e3, 1), "frac_of_8tbs": round(e["bytes"] / e["us"] / 1e3 / 8000.0, 4),
                                         "launches_per_step": round(e["launches_per_step"], 2)} for k, e in sorted(hb.items())}
            result["kernels_hbm_note"] = ("1024 rays are 256 workgroups of four rays: these kernels are latency-bound (one round of short workgroups), "
                                          "not bandwidth-bound; together they are < 2 % of the step")
            big = sorted(((v["us"] * v["n"], k, v) for k, v in live.items() if v.get("clock_ghz")), reverse=True)[:6]
            result["clocks_ghz"] = {_short(k): round(v["clock_ghz"], 3) for _, k, v in big}
            result["step_hbm_bytes"] = round(sum((v["fetch"] + v["write"]) * v.get("n", 0.0) for v in live.values()))
            # north_star: "MFMA utilisation on the MLP GEMMs against gfx950 peak" -- matrix-pipe occupancy of every MFMA kernel from the SQ pass
            # (kernels serialised; with point ranges a per-point kernel is a half-batch launch, 1.56 rounds of workgroups alone on the chip)
            result["kernels_mfma"] = {_short(k): {"mfma_busy": round(v["mfma_busy"], 3), "waves_parked": round(v.get("waves_parked", 0.0), 3),
                                                  "us_per_launch": round(v.get("us", 0.0), 1), "launches_per_step": round(v.get("n", 0.0), 2)}
                                      for k, v in sorted(live.items(), key=lambda kv: -kv[1].get("us", 0.0) * kv[1].get("n", 0.0)) if v.get("mfma_busy", 0.0) > 0.01}
        if weak is not None and strong is not None:
            Bs = strong["rays_per_gpu"]
            result["strong"] = {"value": round(Bs * world * n_shaded / (strong["dt"] / K), 1), "unit": "ray-samples/s", "scaling": "strong",
                                "ms_per_step": round(strong["dt"] / K * 1e3, 4), "windows_ms_per_step": [round(x / K * 1e3, 4) for x in strong["dts"]],
                                "us_per_ray": round(strong["dt"] / K / Bs * 1e6, 4), "global_rays": Bs * world, "rays_per_gpu": Bs, "n_gpus": world}
            result["us_per_ray"] = round(dt / K / head_B * 1e6, 4)
        if world > 1:
            # one line must show a straggler or a transport fallback: the same windows as seen by the slowest and the fastest
            # rank, and the rank count the library's RCCL communicator itself reports (None: torch.distributed carried the collective)
            mins = head.get("dts_rank_min") or head["dts"]
            comm = getattr(getattr(wl.net, "dp_state", None), "comm", None)
            result["ranks"] = {"ms_per_step_slowest_rank": round(sorted(head["dts"])[len(head["dts"]) // 2] / K * 1e3, 4),
                               "ms_per_step_fastest_rank": round(sorted(mins)[len(mins) // 2] / K * 1e3, 4),
                               "windows_ms_per_step_fastest_rank": [round(x / K * 1e3, 4) for x in mins],
                               "rccl_nranks": (comm.nranks() if comm is not None and hasattr(comm, "nranks") else None),
                               "torch_world_size": dist.get_world_size(), "transport": "library RCCL communicator" if comm is not None else "torch.distributed (" + str(args.backend) + ")"}
        result.update(extras)
        if not args.no_extras and world == 1:
            result["eager_rocm_baseline"] = eager_rocm_baseline(dev, iters, n_shaded)
        if not args.no_cpu_baseline and world == 1:
            result["cpu_baseline"] = cpu_baseline(args, iters, n_shaded)
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def full_image(wl, dev, n_shaded, H=480, W_=640, chunk=12000, reps=3):
    """BASELINE.json configs[3] on one GPU: one full 640x480 eval render, all chunks of split_n_pixels = 12000 rays in ONE library call
    (i2sdf_render_image; model/eval/recon.py:161-182, utils/__init__.py:35-84), eval mode, the sampler's data-dependent loop per chunk."""
    import torch
    net = wl.net
    was_training = net.training
    net.eval()
    k_saved, net.force_iters = net.force_iters, 0
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W_), indexing="ij")
    uv = torch.stack([xs, ys], -1).float().reshape(1, -1, 2).to(dev)
    K4 = torch.eye(4); K4[0, 0] = K4[1, 1] = 600.0; K4[0, 2] = W_ / 2; K4[1, 2] = H / 2
    pose = torch.eye(4); pose[:3, 3] = torch.tensor([0.0, 0.0, -2.0])
    inp = {"uv": uv, "intrinsics": K4.unsqueeze(0).to(dev), "pose": pose.unsqueeze(0).to(dev)}
    ts = []
    with torch.no_grad():
        out = net.render_image(inp, split_n_pixels=chunk)
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = net.render_image(inp, split_n_pixels=chunk)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    its = net.last_sampler_iters.tolist()
    net.force_iters = k_saved
    net.train(was_training)
    med = sorted(ts)[len(ts) // 2]
    return {"value": round(H * W_ * n_shaded / med, 1), "unit": "ray-samples/s", "s_per_image": round(med, 4), "images_s": [round(x, 4) for x in ts],
            "rays_per_s": round(H * W_ / med, 1), "chunks": (H * W_ + chunk - 1) // chunk, "sampler_iters_per_chunk": [int(i) for i in its],
            "finite": bool(torch.isfinite(out["rgb_values"]).all() and torch.isfinite(out["normal_map"]).all()),
            "workload": f"BASELINE cfg 4 on one GPU: {W_}x{H} eval render ({H * W_} rays in {(H * W_ + chunk - 1) // chunk} chunks of {chunk}), "
                        f"error-bounded up-sampling with the data-dependent loop per chunk, {n_shaded} shaded samples per ray, one i2sdf_render_image call"}


def allreduce_alone(wl, dev, world, reps=20):
    """The one collective of a training step, timed alone: the mean of the flat gradient buffer over the ranks (3.2 MB), through whatever
    transport attach_data_parallel chose (library RCCL communicator: i2sdf_allreduce_grads; else torch.distributed).  At N = 1 there is
    no collective: the record says so instead of reporting a number."""
    import torch
    net = wl.net
    flat = getattr(net, "_flat", None)
    n = int(flat.numel()) if flat is not None else 0
    if world == 1 or net.grad_sync is None or flat is None:
        return {"value": None, "unit": "us", "bytes": n * 4, "note": "one rank: no collective in the step (the hook is installed by attach_data_parallel for N > 1)"}
    buf = torch.zeros_like(flat)
    for _ in range(3):
        net.grad_sync(buf)
    wl.fence()
    t0 = time.perf_counter()
    for _ in range(reps):
        net.grad_sync(buf)
    wl.fence()
    us = (time.perf_counter() - t0) / reps * 1e6
    t = torch.tensor([us], dtype=torch.float64, device=dev)
    if world > 1:
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    st = getattr(net, "dp_state", None)
    return {"value": round(float(t.item()), 2), "unit": "us", "bytes": n * 4, "reps": reps,
            "transport": "library RCCL communicator (i2sdf_allreduce_grads)" if getattr(st, "comm", None) is not None else "torch.distributed.all_reduce",
            "note": f"mean of {reps} back-to-back all-reduces of the flat fp32 gradient buffer, max over ranks; in a step it runs once, behind the weight-norm backward"}


def dominant_kernel(live, cfg, fp, eng, B, M_main, M_sdf, iters, PEAK, PEAK_BF16):
    """The single rocprofv3 kernel with the largest share of a step's kernel time (the entry-point figure above it prices a whole
    C-ABI call, which may be several kernels): algorithmic FLOPs per step of THAT kernel (SURVEY 8d per-point figures x points)
    / its summed duration in the PMC pass (kernels serialised there: each launch alone on the chip), against the MFMA roof of its arithmetic."""
    sdf = cfg.sdf.dims
    mac_fwd_hidden = sum(o * i for o, i in sdf[:-1])
    per_step = {   # kernel-name fragment -> (algorithmic FLOPs per step, bf16 MFMAs per fp32 product block (0 = fp32-input MFMA))
        "sdf_fwd3h_kernel": (fp["sdf_forward"] * B * cfg.sampler.N_samples_eval * iters, 3 if getattr(eng, "sampler_bf16x2", False) else 6),
        "sdf_fwd3_kernel": (fp["sdf_forward"] * B * cfg.sampler.N_samples_eval * iters, 6),
        "sdf_fwd4_kernel": (fp["sdf_forward"] * B * cfg.sampler.N_samples_eval * iters, 6),
        "sdf_train_fwd3h_kernel": (2 * (mac_fwd_hidden + sdf[-1][0] * sdf[-1][1]) * M_sdf, 6),
        "sdf_igrad3_kernel": ((fp["sdf_forward_grad"] - 2 * (mac_fwd_hidden + sdf[-1][0] * sdf[-1][1])) * M_sdf, 6),
        "sdf_bwd3_sweep1_kernel": (2 * mac_fwd_hidden * M_sdf, 6),
        "sdf_bwd3_sweep2_kernel": ((fp["sdf_backward"] - 2 * mac_fwd_hidden) * M_sdf, 6),
        "rgb_fwd3h_kernel": (fp["rgb_forward"] * M_main, 6),
        "rgb_bwd3h_kernel": (fp["rgb_backward"] * M_main, 6),
        # the 256x256 blocks: 7 SDF layers x 2 products over all points, the feature block + 4 radiance blocks over the ray samples
        "wgrad3p_kernel": (2 * 65536 * (14 * M_sdf + 5 * M_main), 3 if eng.wgrad_bf16x2 else 6),
        # round 6: blocks + narrow tasks of a range in one grid (the narrow tasks' products, ~3 % of the blocks', are not counted)
        "wgrad_all_kernel": (2 * 65536 * (14 * M_sdf + 5 * M_main), 3 if eng.wgrad_bf16x2 else 6),
    }
    best = None
    for k, v in live.items():
        t = v.get("us", 0.0) * v.get("n", 0.0)
        if t > 0 and (best is None or t > best[0]):
            best = (t, k, v)
    if best is None:
        return None
    tot_us = sum(v.get("us", 0.0) * v.get("n", 0.0) for v in live.values())
    t, k, v = best
    short = _short(k)
    rec = {"kernel": short, "us_per_launch": round(v["us"], 1), "launches_per_step": round(v["n"], 2), "share_of_kernel_time": round(t / tot_us, 4),
           "mfma_busy": round(v.get("mfma_busy", 0.0), 3) or None, "hbm_bytes_per_launch": round(v["fetch"] + v["write"]),
           "hbm_gbs": round((v["fetch"] + v["write"]) / v["us"] / 1e3, 1) if v["us"] > 0 else None,
           "source": "the rocprofv3 --pmc passes of this run (kernels serialised: a ranged kernel is a half-batch launch alone on the chip)"}
    for frag, (flops, nmf) in per_step.items():
        if frag in short:
            ach = flops / (t * 1e-6) / 1e12
            peak = PEAK_BF16 / nmf if nmf else PEAK
            rec.update({"algorithmic_flops_per_step": int(flops), "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4)})
            break
    return rec


ENTRY_KERNELS = {"i2sdf_weight_grads": ("wgrad", "wn_backward"), "i2sdf_sdf_backward": ("sdf_bwd",), "i2sdf_sdf_forward_grad": ("sdf_train_fwd", "sdf_igrad"),
                 "i2sdf_sample_rays": ("sdf_fwd", "sampler_"), "i2sdf_rgb_forward": ("rgb_fwd",), "i2sdf_rgb_backward": ("rgb_bwd",),
                 "i2sdf_composite_forward": ("composite_fwd",), "i2sdf_composite_backward": ("composite_bwd", "beta_reduce")}


def source_hash():
    """sha256 over the kernel sources + the C header: what a committed profile must have been taken with to describe this build."""
    import glob
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(here, "i2sdf_amd", "csrc", "*.h*")) + glob.glob(os.path.join(here, "i2sdf_amd", "csrc", "*.cpp"))
                    + [os.path.join(here, "include", "i2sdf.h")]):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def live_traffic(args):
    """HBM traffic per kernel, measured NOW: two rocprofv3 passes (counters only, one --pmc set per run as the profiling guide
    prescribes: FETCH_SIZE [+ GRBM_GUI_ACTIVE for the clock], then WRITE_SIZE) over a short run of the headline workload (this script
    with --pmc-child).  -> {kernel name: {"fetch": bytes/dispatch (FETCH_SIZE x 1024 x 2: the counter tallies 128-B requests of wide
    loads at 64 B on gfx950, MI355X_MICROARCH.md), "write": bytes/dispatch, "us": mean duration, "n": dispatches per step, "clock_ghz"}} or None."""
    import csv
    import shutil
    import tempfile
    if args.no_live_traffic or shutil.which("rocprofv3") is None:
        return None
    here = os.path.dirname(os.path.abspath(__file__))
    out = {}
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        with tempfile.TemporaryDirectory(dir="/tmp") as d:
            for tag, counters in (("fetch", ["FETCH_SIZE", "GRBM_GUI_ACTIVE"]), ("write", ["WRITE_SIZE"]),
                                  ("sq", ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAVE_CYCLES", "GRBM_GUI_ACTIVE"])):
                cmd = ["rocprofv3", "--kernel-trace", "--pmc"] + counters + ["-d", d, "-o", tag, "--output-format", "csv", "--", sys.executable,
                       os.path.join(here, "bench.py"), "--pmc-child", "--steps", "2", "--warmup", "1", "--rays", str(args.rays),
                       "--sampler-iters", str(args.sampler_iters), "--fused-adam", str(args.fused_adam), "--bf16x3", str(args.bf16x3)]
                r = subprocess.run(cmd, cwd=here, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
                cc, kt = os.path.join(d, f"{tag}_counter_collection.csv"), os.path.join(d, f"{tag}_kernel_trace.csv")
                if r.returncode != 0 or not os.path.exists(cc) or not os.path.exists(kt):
                    return None
                agg, cnt, seen, dur = {}, {}, set(), {}
                for row in csv.DictReader(open(cc)):
                    k = row["Kernel_Name"]
                    a = agg.setdefault(k, {})
                    a[row["Counter_Name"]] = a.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
                    if row["Dispatch_Id"] not in seen:
                        seen.add(row["Dispatch_Id"])
                        cnt[k] = cnt.get(k, 0) + 1
                for row in csv.DictReader(open(kt)):
                    dur[row["Kernel_Name"]] = dur.get(row["Kernel_Name"], 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
                steps = max([n for k, n in cnt.items() if "wn_backward" in k] or [0])
                if steps == 0:
                    return None
                for k, a in agg.items():
                    e = out.setdefault(k, {"fetch": 0.0, "write": 0.0})
                    if tag == "fetch":
                        e["fetch"] = a.get("FETCH_SIZE", 0.0) * 1024.0 * 2.0 / cnt[k]
                        e["us"] = dur.get(k, 0.0) / cnt[k] / 1e3
                        e["n"] = cnt[k] / steps
                        if e["us"] > 0 and a.get("GRBM_GUI_ACTIVE", 0.0) > 0:
                            e["clock_ghz"] = a["GRBM_GUI_ACTIVE"] / cnt[k] / 8.0 / (e["us"] * 1e3)
                    elif tag == "write":
                        e["write"] = a.get("WRITE_SIZE", 0.0) * 1024.0 / cnt[k]
                    elif a.get("GRBM_GUI_ACTIVE", 0.0) > 0 and a.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) > 0:
                        # matrix-pipe occupancy: busy cycles summed over the SIMDs / (1024 SIMDs x elapsed cycles); GRBM_GUI_ACTIVE is
                        # the elapsed cycles summed over the 8 XCDs, so 1024 x cycles = 128 x GRBM_GUI_ACTIVE (PMC tables)
                        e["mfma_busy"] = a["SQ_VALU_MFMA_BUSY_CYCLES"] / (128.0 * a["GRBM_GUI_ACTIVE"])
                        if a.get("SQ_WAVE_CYCLES", 0.0) > 0:
                            e["waves_parked"] = a.get("SQ_WAIT_ANY", 0.0) / a["SQ_WAVE_CYCLES"]
        return out or None
    except Exception:
        return None


def _short(kernel_name):
    """'void (anonymous namespace)::sdf_fwd3_kernel<256, 6>(float const*, ...)' -> 'sdf_fwd3_kernel'"""
    import re
    m = re.findall(r"([A-Za-z_][A-Za-z_0-9]*)\s*(?:<[^()]*>)?\s*\(", kernel_name)
    m = [x for x in m if x not in ("void", "anonymous", "namespace")]
    return m[0] if m else kernel_name[:40]


def entry_traffic(live, entry):
    """bytes per step of all kernels of an entry point from live_traffic()"""
    pat = ENTRY_KERNELS.get(entry)
    if not live or not pat:
        return None
    tot = sum((v["fetch"] + v["write"]) * v.get("n", 0.0) for k, v in live.items() if any(q in k for q in pat))
    return round(tot) if tot > 0 else None


def profiled_traffic(entry):
    """Fallback when rocprofv3 is not on PATH: HBM bytes per launch of an entry point from the newest committed PMC summaries
    (profiles/r*_pmc_{fetch,write}_summary.csv), accepted only if profiles/r*_source_hash.txt matches this build's sources
    (a profile of other kernels would silently describe the wrong code).  -> (bytes | None, source label)."""
    import csv
    import glob
    pat = ENTRY_KERNELS.get(entry)
    here = os.path.dirname(os.path.abspath(__file__))
    rounds = sorted({os.path.basename(p).split("_")[0] for p in glob.glob(os.path.join(here, "profiles", "r*_pmc_fetch_summary.csv"))},
                    key=lambda r: int(r[1:]) if r[1:].isdigit() else -1)
    if not rounds or not pat:
        return None, None
    tag_r = rounds[-1]
    try:
        stamp = open(os.path.join(here, "profiles", f"{tag_r}_source_hash.txt")).read().split()[0]
    except (OSError, IndexError):
        stamp = None
    if stamp != source_hash():
        return None, f"profiles/{tag_r}_pmc_* were taken with other kernel sources (hash {stamp}, this build {source_hash()}): not used"
    try:
        tot = 0.0
        for tag, col, mult in (("fetch", "FETCH_SIZE_per_dispatch", 2.0), ("write", "WRITE_SIZE_per_dispatch", 1.0)):
            rows = list(csv.DictReader(open(os.path.join(here, "profiles", f"{tag_r}_pmc_{tag}_summary.csv"))))
            steps = max([int(r["dispatches"]) for r in rows if "wn_backward" in r["kernel"]] or [0])
            if steps == 0:
                return None, None
            tot += sum(float(r[col]) * 1024.0 * mult * int(r["dispatches"]) for r in rows if any(q in r["kernel"] for q in pat)) / steps
        return (round(tot), f"profiles/{tag_r}_pmc_{{fetch,write}}_summary.csv (committed rocprofv3 --pmc passes of this build's sources, not measured in this run)") \
            if tot > 0 else (None, None)
    except (OSError, KeyError, ValueError):
        return None, None


def _oracle_case(Bc, iters, n_shaded, device, dtype_seed=7):
    import torch
    from oracle import i2sdf_oracle as orc
    ocfg = orc.synthetic_cfg(False)
    ocfg.use_normal = True
    sd = orc.init_params(ocfg, seed=0)
    sd["density.beta"] = torch.tensor(0.02)
    g = torch.Generator().manual_seed(dtype_seed)
    K = torch.eye(4); K[0, 0] = K[1, 1] = 600.0; K[0, 2] = 320.0; K[1, 2] = 240.0
    pose = torch.eye(4); pose[:3, 3] = torch.tensor([0.0, 0.0, -2.0])
    uv = torch.stack([torch.randint(0, 640, (Bc,), generator=g), torch.randint(0, 480, (Bc,), generator=g)], -1).float().reshape(Bc, 1, 2)
    inp = {"uv": uv, "intrinsics": K.repeat(Bc, 1, 1), "pose": pose.repeat(Bc, 1, 1)}
    gt = {"rgb": torch.rand(Bc, 3, generator=g), "depth": torch.rand(Bc, generator=g) * 3, "depth_mask": torch.ones(Bc, dtype=torch.bool),
          "normal": torch.nn.functional.normalize(torch.randn(Bc, 3, generator=g), dim=1), "normal_mask": torch.ones(Bc, dtype=torch.bool)}
    sc = ocfg.sampler
    R = ocfg.scene_bounding_sphere
    dr = orc.Draws(strat_u=torch.rand(Bc, sc.N_samples_eval, generator=g), cdf_u=torch.rand(Bc, sc.N_samples, generator=g),
                   extra_idx=torch.randperm(sc.N_samples_eval * max(iters, 1), generator=g)[: sc.N_samples_extra],
                   eik_idx=torch.randint(n_shaded + 1, (Bc,), generator=g), eik_pts=(torch.rand(Bc, 3, generator=g) * 2 - 1) * R,
                   nbr_off=(torch.rand(Bc, 3, generator=g) * 2 - 1) * 0.005)
    lc = orc.LossCfg(eikonal_weight=0.1, smooth_weight=0.01, smooth_iter=150000, depth_weight=0.1, normal_weight=0.05)
    mv = lambda d: {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in d.items()}
    dr = orc.Draws(**mv(vars(dr)))
    return orc, ocfg, mv(sd), mv(inp), mv(gt), lc, dr


def cpu_probe(spec):
    """child mode (--cpu-probe threads,rays,k,n_shaded): time the CPU restatement with `threads` torch threads, print one JSON line"""
    import torch
    threads, Bc, iters, n_shaded = (int(x) for x in spec.split(","))
    torch.set_num_threads(threads)
    orc, ocfg, sd, inp, gt, lc, dr = _oracle_case(Bc, iters, n_shaded, "cpu")
    times = []
    for i in range(4):
        t0 = time.perf_counter()
        orc.training_step_grads(sd, ocfg, inp, gt, lc, dr, step=10, force_iters=iters or None)
        times.append(time.perf_counter() - t0)
        print(json.dumps({"threads": threads, "rays": Bc, "times": times}), flush=True)     # a line per step: a killed child still reports
        if sum(times) > 30.0 and len(times) >= 2:
            break


def _cpu_case(threads, Bc, iters, n_shaded, timeout):
    """One bounded measurement in a child process (torch's intra-op thread count cannot be changed reliably once used, and an
    over-subscribed run must be killable): -> dict(value, s_per_step, steps) or dict(value None, note)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-probe", f"{threads},{Bc},{iters},{n_shaded}"]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(threads))
    last = None
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=timeout)
        lines = r.stdout.decode().strip().splitlines()
    except subprocess.TimeoutExpired as e:
        lines = (e.stdout or b"").decode().strip().splitlines()
    for ln in lines:
        try:
            last = json.loads(ln)
        except ValueError:
            pass
    if not last or not last.get("times"):
        return {"value": None, "threads": threads, "rays": Bc, "note": f"no step of {Bc} rays finished within {timeout} s"}
    t = last["times"]
    timed = t[1:] if len(t) > 1 else t               # first step = warm-up when there is a second one
    med = sorted(timed)[len(timed) // 2]
    return {"value": round(Bc * n_shaded / med, 1), "threads": threads, "rays": Bc, "s_per_step": round(med, 3),
            "steps": f"median of {len(timed)} timed step(s)" + (" after 1 warm-up" if len(t) > 1 else " (no warm-up: the first step hit the time bound)")}


def cpu_baseline(args, iters, n_shaded):
    """The CPU oracle (a port of the reference's PyTorch path, validated against it) timed on this node's host cores on bounded
    samples of the same workload (same networks, same camera, same fixed k, fewer rays), SURVEY 8(d): with n = all physical cores,
    with n = 1, and with the thread count torch's CPU GEMMs on 256-wide layers actually scale to (32) -- the best of them is `value`.
    Every case is a child process with a time bound, so the default run stays within minutes on any host."""
    ncpu = os.cpu_count() or 1
    phys = ncpu
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or ncpu
    except Exception:
        pass
    cases = {"best_of_threads_32": _cpu_case(min(ncpu, 32), args.cpu_rays, iters, n_shaded, 60),
             "one_thread": _cpu_case(1, 16, iters, n_shaded, 45),
             "all_physical_cores": _cpu_case(phys, 64, iters, n_shaded, 45)}
    best = max((c for c in cases.values() if c.get("value")), key=lambda c: c["value"], default=None)
    out = {"value": best["value"] if best else None, "unit": "ray-samples/s", "cores": best["threads"] if best else 0, "kind": "port",
           "sample": (f"{best['rays']} rays x {n_shaded} shaded samples, same nets/camera/k={iters}, fwd+loss+bwd (no optimizer), torch CPU fp32, "
                      f"{best['threads']} threads, {best['steps']}, {best['s_per_step']} s/step") if best else "no case finished",
           "host": {"os_cpu_count": ncpu, "physical_cores": phys},
           "cases": cases,
           "note": "torch's CPU GEMMs on 256-wide layers stop scaling beyond a few tens of threads and collapse under over-subscription "
                   "(round 2, all 256 hardware threads: 108.8 s per 64-ray step); every case here is bounded in time"}
    return out


def eager_rocm_baseline(dev, iters, n_shaded, Bc=1024):
    """The un-fused GPU baseline of BASELINE.md section 3: the CPU restatement's own torch ops (autograd double backward
    included) run as stock PyTorch-ROCm eager kernels on this MI355X, same nets/camera/k, fwd+loss+bwd, no optimizer."""
    import torch
    try:
        orc, ocfg, sd, inp, gt, lc, dr = _oracle_case(Bc, iters, n_shaded, dev)
        times = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            orc.training_step_grads(sd, ocfg, inp, gt, lc, dr, step=10, force_iters=iters or None)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        med = sorted(times[1:])[len(times[1:]) // 2]
        return {"value": round(Bc * n_shaded / med, 1), "unit": "ray-samples/s", "kind": "port on stock PyTorch-ROCm eager ops (fp32, no TF32 on gfx950)",
                "sample": f"{Bc} rays x {n_shaded} shaded samples, k={iters}, median of 3 after 1 warm-up, {med * 1e3:.1f} ms/step"}
    except Exception as e:          # the oracle is CPU-first test infrastructure; a device-placement slip must not kill the headline
        return {"value": None, "error": f"{type(e).__name__}: {e}"[:300]}


if __name__ == "__main__":
    main()
