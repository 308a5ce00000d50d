#!/usr/bin/env python3
"""bench.py — Msamples/s (ray·bounces = closest-hit segments per second) of the per-pixel sample loop on MI355X.

  python bench.py --gpus 1 --steps K --warmup W [--workload cfg3|cfg2|cfg5] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one full frame of the workload (every pixel, every sample, all bounces).  Default workload = cfg3 of
BASELINE.json — the 1 000 000-triangle mesh + HDRI IBL at 1920x1080, 512 spp, depth 10 — because that is the
configuration the metric's roofline target ("1M-triangle BVH traversal at 1 GPU") and the multi-GPU config (cfg4,
"same 1M-tri scene pixel-tiled") are quoted on; cfg2 (configs[1]) and cfg5 are selectable with --workload.
With N > 1 the frame's 32x32 pixel tiles are interleaved over the ranks (scene replicated, weak in memory but the
total work is fixed => "strong" scaling) and every step ends with one RCCL gather of the ranks' packed tiles (1/N of the
double3 accumulator each) onto rank 0, which scatters them into the frame.  `python bench.py --gpus N` without a launcher starts
its N ranks itself (fresh child processes through torch.distributed.run, before anything touches the GPU).

The timed region starts with the scene (BVH, vertices, normals, HDRI) resident in HBM and contains: zeroing the
accumulator, the render kernel(s), the RCCL exchange.  One JSON line is printed by rank 0.

A plain run does what the headline needs: it builds and commits the scene once, renders one counting step (the segment
count the headline divides by comes from it; the roofline is priced on the same counts and on the timed launches),
warms up, times the steps, writes the frame with --dump-outputs and prints the line.  --full adds what takes runs of
its own: a second commit, whose time is the restart cost (`config.bvh_build_upload_s`, null without --full), and the
CPU baseline (`cpu_baseline`: the reference and the CPU restatement on host cores, about 65 s on cfg3).
"""
import argparse
import glob
import hashlib
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RANDOM_RECORD_PEAK_G = 60.0   # G dependent random records/s beyond L2, measured on MI355X by scripts/dev/randread.hip (profiles/README.md)
RANDOM_RECORD_L2_G = 206.0    # ... from an L2-resident array (same microbenchmark, 64-byte records)


def record_peak(l2_hit):
    """the rate the chip serves dependent random records at for a given L2 hit rate: the harmonic blend of the two measured rates; without a counter
    file the all-miss rate (the kernel then reads above 1.0 of it whenever part of its records hit L2: that is what the blend corrects)"""
    if l2_hit is None:
        return RANDOM_RECORD_PEAK_G
    return 1.0 / (l2_hit / RANDOM_RECORD_L2_G + (1.0 - l2_hit) / RANDOM_RECORD_PEAK_G)
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
FP64_PEAK_FLOPS = 256 * 4 * 16 * 2 * 2.4e9   # FP64 vector: 256 CUs x 4 SIMDs x 16 lanes x 2 flops (FMA) x 2.4 GHz = 78.6 TFLOP/s
VALU_ISSUE_PEAK_G = 256 * 4 * 2.4e9 / 4 * 1e-9   # vector issue: 1024 SIMDs, a wave64 instruction occupies its SIMD for 4 cycles, 2.4 GHz = 614.4 G wave-instructions/s


def kernel_src_sha():
    """identifies the kernel + host sources a counter pass was taken on (profiles/*_traffic.json carry it)"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "raytracer_project_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h", ".cpp")) and f != "zr_scenes_lib.cpp":
            h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def _round_key(path):
    m = re.match(r"r(\d+)_?(.*)", os.path.basename(path))
    return (int(m.group(1)), m.group(2)) if m else (0, "")

WORKLOADS = {
    "cfg3": ("cfg3", (), "1M-triangle torus-knot mesh + 4096x2048 HDRI IBL, 1920x1080, 512 spp, depth 10"),
    "cfg2": ("cfg2", (), "Shirley random spheres (485 spheres), 1280x720, 256 spp, depth 50"),
    "cfg5": ("cfg5", (), "Cornell box: cubes + constant_medium + dielectric, 600x600, 1024 spp, depth 50"),
    "cfg1": ("cfg1", (), "3 Lambertian spheres, 400x225, 16 spp, depth 8"),
    "cfg3w": ("cfg3w", (), "cfg3 with the mesh placed as the reference places meshes: 1M triangles under material_instance -> rotate_x -> "
                           "rotate_z -> translate, 1920x1080, 512 spp, depth 10"),
    "demo": ("demo", (), "the reference's demo workload (scene_management.hpp:103-236): ~900 scaled/rotated/re-materialed instances, "
                         "a wrapped 3840-triangle mesh, fog volume, 1280x720, 128 spp, depth 10"),
}
# bounded CPU-baseline samples (xstep, spp): every xstep-th column of EVERY row of the frame at spp samples per pixel, sized for
# ~10-30 s on 16 host threads; xstep divides every workload's width, so that the restatement can render exactly the same pixel
# set through the C ABI's region (tile_size 1, tile_mod xstep)
CPU_SAMPLE = {"cfg3": (8, 64), "cfg2": (8, 192), "cfg5": (8, 128), "cfg1": (1, 16), "demo": (8, 96), "cfg3w": (8, 64)}


def host_threads():
    """threads this process may use: its CPU affinity (the GPU box hands a 1-GPU job a share of the host), all of them"""
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except Exception:
        return max(1, os.cpu_count() or 1)


def cpu_baseline(workload):
    """The reference's CPU arithmetic (oracle/_ref: genuine headers compiled in the build container) on a bounded sample of the
    same workload at its best thread count (median of 3) and on all host cores this process may use, and the CPU restatement
    (oracle/libzr_oracle.so, "port") on the same pixels and samples beside it."""
    from oracle import zr_oracle_py as zo
    from raytracer_project_amd import capi
    xs, spp = CPU_SAMPLE[workload]
    scene = WORKLOADS[workload][0]
    threads = host_threads()
    # the restatement: same pixels (every xs-th column of every row), same spp, same seeds
    ds = capi.DemoScene(scene)
    cam = ds.camera.copy()
    cam.samples_per_pixel = spp
    osc = zo.OracleScene(ds.desc)
    reg = capi.Region(0, 0, 0, 0, 1, xs, 0, 0) if xs > 1 else None
    t0 = time.perf_counter()
    frame, ctr, _, _ = osc.render(cam, ds.env, ds.seed, reg, threads=threads)
    dt = time.perf_counter() - t0
    port = {"value": round(ctr.segments / dt * 1e-6, 4), "unit": "Msamples/s", "cores": threads, "kind": "port",
            "sample": f"every {xs}th column of every row at {spp} spp ({ctr.primary_samples} primary samples, {ctr.segments} segments, {dt:.1f} s); "
                      "own flattened BVH (SAH), thread-local counter RNG"}
    if not zo.ref_available():
        port["host_cores"] = os.cpu_count()
        return port
    # The reference at its BEST thread count is the headline: its hit_record copies a shared_ptr<material> per candidate, whose
    # refcounts ping-pong between cores, so on a many-core host it is faster at 16 threads than on all of them (measured: 4.1 against
    # 2.2 Msamples/s on the 256-thread box).  Median of 3 runs at 16 threads; one run on all cores is printed beside it.
    best_threads = min(16, threads)
    runs = sorted((zo.ref_run("time", scene, xs, 1, spp, best_threads) for _ in range(3)), key=lambda q: q["mseg_per_s"])
    r = runs[1]
    same = r["segments"] == ctr.segments and abs(float(frame.sum()) - r["checksum"]) <= 1e-9 * max(1.0, abs(r["checksum"]))
    every = None
    if threads > best_threads:
        ra = zo.ref_run("time", scene, xs, 1, spp, threads)
        every = {"value": round(ra["mseg_per_s"], 4), "cores": threads, "render_s": round(ra["render_s"], 1)}
    return {"value": round(r["mseg_per_s"], 4), "unit": "Msamples/s", "cores": best_threads, "kind": "reference", "host_cores": os.cpu_count(),
            "runs": [round(q["mseg_per_s"], 4) for q in runs],
            "sample": f"every {xs}th column of every row of the frame at {spp} spp ({r['primary']} primary samples, "
                      f"{r['segments']} segments, {r['render_s']:.1f} s, median of 3; the reference's median-split BVH build, {r['bvh_build_s']:.1f} s, is not counted); "
                      "genuine reference hit / scatter / BVH / camera functions with the per-(pixel, sample) counter RNG in place of its "
                      "shared mt19937 (no cache-line ping-pong between threads on the engine: this number flatters the reference), rows dealt to "
                      f"{best_threads} threads dynamically — the reference's best thread count on this host",
            "reference_on_all_cores": every, "port": port, "port_matches_reference": bool(same)}


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves — as FRESH child processes, before this
    process has touched the GPU (an exec or a fork after a HIP call is not allowed on this pool) — through
    torch.distributed.run on 127.0.0.1, relay rank 0's JSON line and exit with the launcher's code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL between processes needs it on this host driver
    env.setdefault("OMP_NUM_THREADS", "1")
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in p.stdout:   # rank 0's JSON line goes to stdout; whatever else the ranks or their libraries print (gloo's connection notes) to stderr
        (sys.stdout if line.startswith("{") else sys.stderr).write(line)
    raise SystemExit(p.wait())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="cfg3", choices=sorted(WORKLOADS))
    ap.add_argument("--spp", type=int, default=0, help="override samples per pixel (invalidates the headline number)")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: the restart commit and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--kernel-src-sha", action="store_true", help="print the source hash profiles/*_traffic.json are keyed by, and exit")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the frame the last step computed to DIR/radiance.npy")
    args = ap.parse_args()
    if args.kernel_src_sha:
        print(kernel_src_sha())
        return
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and os.environ.get("ZR_BENCH_SHARD_OF"):
        ap.error("--dump-outputs needs the whole frame: ZR_BENCH_SHARD_OF renders one rank's tiles only")

    if args.gpus > 1 and "RANK" not in os.environ:   # started plainly, like the N = 1 case: be our own launcher
        self_launch(args.gpus)

    import torch
    from raytracer_project_amd import capi, multi

    rank, local, world = multi.init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    if world > 1 and not os.environ.get("ZR_BENCH_ONE_DEVICE") and torch.cuda.device_count() < world:
        raise SystemExit(f"--gpus {world} but this node shows {torch.cuda.device_count()} device(s) "
                         "(ZR_BENCH_ONE_DEVICE=1 ZR_DIST_BACKEND=gloo rehearses the N-rank path on one GPU)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (there is no CPU path)")
    if os.environ.get("ZR_BENCH_ONE_DEVICE"):   # rehearsal of the N > 1 path on a one-GPU box (gloo): every rank on device 0
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    scene_name, scene_args, descr = WORKLOADS[args.workload]
    t0 = time.perf_counter()
    sys.stdout.flush()
    saved_stdout = os.dup(1)      # the drop-in's `model` announces itself on std::cout like the reference's (model.hpp:103):
    os.dup2(2, 1)                 # keep this process's stdout to the one JSON line
    try:
        ds = capi.DemoScene(scene_name, *scene_args)
    finally:
        os.dup2(saved_stdout, 1); os.close(saved_stdout)
    t_scene = time.perf_counter() - t0
    cam = ds.camera.copy()
    if args.spp > 0:
        cam.samples_per_pixel = args.spp
    ctx = capi.Context(local)
    t0 = time.perf_counter()
    sc = capi.Scene(ctx, ds.desc)           # BVH build + upload: reported, not timed
    t_commit_first = time.perf_counter() - t0
    t_commit = None
    if args.full:
        # the reference rebuilds its BVH on every render restart (main.cpp:1492-1500): what a restart costs is a commit in a process that
        # has committed before (the first one also loads the code objects and warms the allocator); both are reported
        sc.close()
        t0 = time.perf_counter()
        sc = capi.Scene(ctx, ds.desc)
        t_commit = time.perf_counter() - t0
    stats = sc.stats()

    H, W = cam.image_height, cam.image_width
    if args.dump_outputs and H * W * 3 * 8 > 64 * 10**6:
        raise SystemExit(f"--dump-outputs: the {W}x{H} float64 frame is over the 64 MB the dump may hold")
    acc = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    region = multi.tile_region(capi, rank, world)
    if os.environ.get("ZR_BENCH_SHARD_OF"):  # development aid: time one rank's share of an N-way sharded frame on one GPU
        region = multi.tile_region(capi, int(os.environ.get("ZR_BENCH_SHARD_RANK", "0")), int(os.environ["ZR_BENCH_SHARD_OF"]))
    stream = torch.cuda.current_stream(dev).cuda_stream

    def step(count=False):
        acc.zero_()
        sc.render_device(cam, ds.env, ds.seed, acc.data_ptr(), stream, region, count)
        multi.exchange_frame(acc, world)

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    # counting pass (instrumented kernel, never timed): segments and algorithmic bytes of one step
    step(count=True)
    torch.cuda.synchronize(dev)
    ctr = ctx.counters()
    seg_local = ctr.segments
    # the dominant kernel of the streaming pipeline is EXTEND (BVH walk): it owns the box / primitive bytes; the 76 B of
    # shading data per hit belong to the SHADE kernel and are left out of the EXTEND roofline
    bytes_local = ctr.algorithmic_bytes() - (76 * ctr.hits if int(getattr(ctr, "path", 2)) in (2, 3) else 0)
    segments, alg_bytes, primary = multi.all_reduce_values([seg_local, bytes_local, ctr.primary_samples], world, dev)
    checksum = float(acc.sum().item()) if rank == 0 else 0.0

    for _ in range(args.warmup):
        step()
    ctx.kernel_times_ms()  # drain the launch log
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(dev)
    t_own = time.perf_counter()
    barrier()
    dt = time.perf_counter() - t0
    # every rank's own time over the timed steps (render + its side of the exchange, before the closing barrier is counted: taken per rank right after its
    # last step's device work): the spread shows load imbalance between the ranks' tile sets the day the 8-GPU curve is measured
    dt_own = t_own - t0
    per_rank = multi.all_reduce_values([dt_own if r == rank else 0.0 for r in range(world)], world, dev) if world > 1 else [dt_own]
    dt = multi.all_reduce_values([dt], world, dev, op="max")[0]
    launches = ctx.kernel_times_ms(1 << 20)  # dominant kernel's launches (HIP events on the launch stream), timed steps only
    variant = int(os.environ.get("ZR_KERNEL", "2"))
    path = int(getattr(ctr, "path", 2 if variant == 2 else 0))   # which kernels rendered the frame (zr_counters::path)
    kernel_name = {0: "render_pixels", 2: "stream_extend", 3: "fused_render"}.get(path, "render_pixels")

    if rank == 0 and args.dump_outputs:
        import numpy as np
        # the frame a caller of the timed path receives: the per-pixel mean radiance, (H, W, 3) float64, whole (cfg3's 1920x1080 is 49.8 MB).
        # Every input is fixed by the workload (compiled scene, camera, seed), so two builds can be compared output for output
        frame = acc.cpu().numpy()
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "radiance.npy"), frame)
    if rank == 0:
        ms_step = dt / args.steps * 1e3
        value = segments * args.steps / dt * 1e-6
        k_ms = sum(launches) / max(1, len(launches))
        launches_per_step = max(1, len(launches) // max(1, args.steps))
        # roofline of the dominant kernel: this rank's algorithmic bytes per launch / mean launch duration
        # (= bytes of one step / summed duration of that kernel's launches in one step)
        achieved = (bytes_local / launches_per_step) / (k_ms * 1e-3) * 1e-9 if k_ms > 0 else 0.0
        # the same traversal priced on THIS layout (what a no-reuse walk of the stored data would move): 64 B per 4-wide node
        # fetched (the root's four boxes travel in the kernel arguments), 72 B / 32 B / 48 B per triangle / sphere / cube tested
        layout_bytes = (64 * ctr.node_lanes + 72 * ctr.triangles_tested + 32 * ctr.spheres_tested + 48 * ctr.cubes_tested) if path == 2 else None
        achieved_layout = (layout_bytes / launches_per_step) / (k_ms * 1e-3) * 1e-9 if (layout_bytes and k_ms > 0) else None
        # counter passes of the dominant kernel from the newest committed file of THIS kernel source (separate --pmc runs:
        # scripts/profile_round.sh); a pass taken on other sources is stale and reported as null
        traffic, traffic_file, kj = None, None, {}
        if world == 1 and args.spp == 0:
            for f in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_{args.workload}_traffic.json")), key=_round_key, reverse=True):
                try:
                    tj = json.load(open(f))
                    if tj.get("workload") != args.workload or tj.get("kernel_src_sha") != kernel_src_sha():
                        continue
                    kj = tj["kernels"][kernel_name]
                    traffic = int(kj["hbm_read_bytes_per_launch"] + kj.get("hbm_write_bytes_per_launch", 0))   # reads (x2 corrected) + writes
                    traffic_file = os.path.relpath(f, ROOT)
                    break
                except Exception:
                    kj = {}
                    continue
        sub_pools = int(round(launches_per_step / max(1, int(getattr(ctr, "rounds", 0)) or launches_per_step))) if path == 2 else 1
        node_util = ctr.node_lanes / max(1, ctr.node_execs) / 64.0
        leaf_util = ctr.leaf_lanes / max(1, ctr.leaf_execs) / 64.0
        # every lane-step of the walk fetches ONE randomly placed record (a 64-B node, a 72-B triangle, a 32-B sphere ...): the
        # rate at which the chip serves dependent random records is what the kernel runs against (scripts/dev/randread.hip, same
        # occupancy: ~60 G records/s from arrays beyond the L2s whatever the record size up to 128 B, ~206 G/s L2-resident)
        records = (ctr.node_lanes + ctr.triangles_tested + ctr.spheres_tested + ctr.cubes_tested + ctr.media_tested) if path == 2 else None
        rec_rate = (records / launches_per_step) / (k_ms * 1e-3) * 1e-9 if (records and k_ms > 0) else None
        # WHAT BOUNDS the dominant kernel, per workload.  From the counter file when one of this kernel source exists (L2 hit rate,
        # FP64 issue), else from the working set: a world whose nodes + primitives fit the 32 MiB of L2 runs out of the caches and is
        # limited by FP64 vector issue; beyond that the walk is limited by the rate at which dependent random records come back
        # through L2 and the fabric.  The fused kernel keeps everything in registers / scalar loads: FP64 issue by construction.
        l2_hit = kj.get("l2_hit_rate")
        valu_issue = kj.get("valu_issue_frac")
        fp64_flops = kj.get("fp64_flops_per_launch")
        fp64_frac = round(fp64_flops / (k_ms * 1e-3) / FP64_PEAK_FLOPS, 4) if (fp64_flops and k_ms > 0) else None
        if path == 3:
            bound, why = "fp64-valu", "fused small-scene kernel: path state in registers, objects through scalar loads; HBM sees 24 B per sample"
        elif stats["device_bytes"] <= 32 * 2**20:
            bound, why = "fp64-valu", f"nodes + primitives ({stats['device_bytes']} B) fit the 8 x 4 MiB of L2: the walk's records are cache hits, the FP64 primitive tests and the pipeline's own state traffic remain"
        else:
            bound, why = "l2-request-rate", (f"nodes + primitives ({stats['device_bytes'] >> 20} MiB) exceed L2: every lane-step fetches one randomly placed record; the kernel moves "
                                            "them at random_record_rate_G_per_s against ~60 G/s beyond L2 / ~206 G/s L2-resident (scripts/dev/randread.hip)")
        if path == 2 and valu_issue is not None and valu_issue >= 0.7:
            # the counters overrule the guess: the walk's vector instructions (FP32 slab tests, the sort of four children, FP64 primitive tests) fill the issue slots
            bound, why = "valu-issue", (f"SQ_INSTS_VALU x 4 cycles fill {100 * valu_issue:.0f} % of the chip's vector issue slots over the kernel's active cycles (1024 SIMDs): the walk executes them at "
                                        f"{100 * node_util:.0f} % / {100 * leaf_util:.0f} % lane utilisation of its NODE / LEAF phases (L2 hit rate {l2_hit}).  Measured at the knee: 6.8 % fewer vector instructions left "
                                        "the duration unchanged, 9 % more cost 10 % (profiles/r3_experiments_ab.txt) - the vector pipe and the walk's fetch path are in balance")
        bound_source = (f"counters: {traffic_file}" if (l2_hit is not None or fp64_frac is not None or valu_issue is not None) else "working set vs L2 (no counter pass of this kernel source committed)")
        # WHICH CEILING `frac` is a fraction of.  A world beyond the L2s is priced against the HBM peak.  A world whose nodes and primitives sit in
        # L2 — or in registers and scalar loads: the fused kernel — is not under that ceiling (round 3 printed 1.10 of it for cfg2): its dominant kernel is limited
        # by vector issue, so `achieved` / `peak` / `frac` are its wave-instructions per second (SQ_INSTS_VALU per launch from the counter file / the launch
        # duration measured here) against the chip's issue rate (1024 SIMDs, one wave64 instruction per 4 cycles at 2.4 GHz); the HBM-model figure stays beside
        # it as `frac_hbm_model`.  Without a counter pass of the current kernel source there is no such figure: `frac` is null, not a fraction of the wrong ceiling.
        hbm_model = {"achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5)}
        in_cache = path == 3 or stats["device_bytes"] <= 32 * 2**20
        insts = kj.get("valu_insts_per_launch")
        if in_cache:
            if insts and k_ms > 0:
                ach = insts / (k_ms * 1e-3) * 1e-9
                headline = {"achieved": round(ach, 2), "peak": VALU_ISSUE_PEAK_G, "unit": "G wave-instructions/s", "frac": round(ach / VALU_ISSUE_PEAK_G, 5)}
                bound = "valu-issue"
            else:
                headline = {"achieved": None, "peak": VALU_ISSUE_PEAK_G, "unit": "G wave-instructions/s", "frac": None}
        else:
            headline = hbm_model
        out = {
            "metric": "Msamples/sec (rays·bounces)", "value": round(value, 3), "unit": "Msamples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "per_rank_ms_per_step": {"min": round(min(per_rank) / args.steps * 1e3, 3), "max": round(max(per_rank) / args.steps * 1e3, 3),
                                     "ranks": [round(x / args.steps * 1e3, 3) for x in per_rank]},
            "config": {"workload": f"{args.workload}: {descr}", "image": [W, H], "spp": cam.samples_per_pixel,
                       "max_depth": cam.max_depth, "segments_per_step": int(segments), "primary_per_step": int(primary),
                       "segments_per_primary": round(segments / max(primary, 1), 4),
                       "parallelism": f"pixel-tiles x{world}" if world > 1 else "single GPU",
                       "bvh_pairs": stats["bvh_pairs"], "bvh_depth": stats["bvh_depth"], "objects": stats["objects"],
                       "traversal_stack": stats.get("traversal_stack"),
                       "scene_build_s": round(t_scene, 3), "bvh_build_upload_s": round(t_commit, 3) if t_commit is not None else None,
                       "bvh_build_upload_first_s": round(t_commit_first, 3),
                       "bvh_builder": stats.get("builder"), "render_path": {0: "pixel-group megakernel", 2: "streaming pipeline", 3: "fused small-scene kernel"}.get(path),
                       "frame_checksum": checksum},
            # `achieved` / `frac`: SURVEY 8(d)'s ALGORITHMIC bytes (a work rate: the no-reuse BVH2-style model) per launch / launch
            # duration against the HBM peak — the figure the contract asks for.  It is NOT memory headroom: `bound` names what the
            # kernel is limited by, `frac_layout` prices the same traversal on the stored layout, `frac_traffic` is what the
            # memory-side counters saw.
            "roofline": {"bound": bound, "bound_why": why, "bound_source": bound_source,
                         "achieved": headline["achieved"], "peak": headline["peak"], "unit": headline["unit"],
                         "frac": headline["frac"], "achieved_hbm_model": hbm_model["achieved"], "frac_hbm_model": hbm_model["frac"], "traffic": traffic,
                         # two sub-pools on two streams (render_stream: worlds whose lean EXTEND and SHADE builds fit side by side): this kernel's launches ran
                         # beside the other pool's SHADE, and their HIP-event durations — hence `achieved` — include that sharing
                         "sub_pools": sub_pools, "co_running": sub_pools > 1,
                         "traffic_source": traffic_file,
                         "frac_traffic": round(traffic / (k_ms * 1e-3) * 1e-9 / HBM_PEAK_GBS, 5) if (traffic and k_ms > 0) else None,
                         "l2_hit_rate": l2_hit,
                         "valu_issue_frac": valu_issue, "fp64_valu_frac": fp64_frac, "fp64_peak_tflops": FP64_PEAK_FLOPS * 1e-12,
                         "achieved_layout": round(achieved_layout, 2) if achieved_layout else None,
                         "frac_layout": round(achieved_layout / HBM_PEAK_GBS, 5) if achieved_layout else None,
                         "random_records_per_launch": int(records / launches_per_step) if records else None,
                         "random_record_rate_G_per_s": round(rec_rate, 2) if rec_rate else None,
                         "random_record_peak_G_per_s": round(record_peak(l2_hit), 1) if records else None,
                         "frac_random_records": round(rec_rate / record_peak(l2_hit), 4) if rec_rate else None,
                         "lane_utilisation": {"node": round(node_util, 3), "leaf": round(leaf_util, 3)} if path == 2 else None,
                         "kernel": kernel_name, "kernel_ms": round(k_ms, 4), "launches_timed": len(launches),
                         "kernel_ms_per_step": round(sum(launches) / max(1, args.steps), 3),
                         "algorithmic_bytes_per_launch": int(bytes_local / launches_per_step),
                         "model": ("32 B per child box tested + 72 B per triangle + 32 B per sphere + 48 B per cube test (SURVEY 8(d) prices a cube at 96 B; this layout stores 6 of "
                                   "its 12 doubles — a placed cube's record is 128 B — so the figure is conservative); the 76 B per hit of shading data belong to SHADE "
                                   "and are NOT in this kernel's figure")},
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(args.workload)
            except Exception as e:  # the baseline is reported, never required
                out["cpu_baseline"] = {"value": None, "unit": "Msamples/s", "cores": 0, "kind": "port", "sample": f"failed: {e}"}
        print(json.dumps(out))
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
