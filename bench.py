#!/usr/bin/env python
"""Benchmark of the MFP train-step hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config c2|c3|c4|c5] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the line: the headline figure and nothing else.  `--full`
adds the checks and extra measurements described below (the median pass, the bf16 / fp8 deviations, the roofline, c5's
fp8 mode, the CPU baseline); `--no-roofline` / `--no-cpu-baseline` leave legs of it out.  `--dump-outputs DIR` writes
what the last timed step handed its caller to DIR/<name>.npy (see dump_outputs); the inputs are seeded, so two builds
run with the same arguments can be compared output for output.

Metric (BASELINE.json): elements/sec of the train step (masking -> forward -> masked losses ->
backward -> [RCCL all-reduce] -> clipnorm + L2 + Keras Adam) on Crello-shaped synthetic batches.
One "element" = one sequence slot of a document.  Inputs are resident in HBM before the timed
region.  For N>1 the driver launches this file under ``python -m torch.distributed.run`` (one rank
per GPU, RCCL); run directly with --gpus N>1 it re-launches itself that way.  Rank 0 prints ONE
JSON line.

Configurations (BASELINE.json `configs`, SURVEY.md section 8 shorthand; documents per GPU are fixed as
N grows = weak scaling):
  c1  RICO masking_method=random, d_model 128, 2 blocks, seq_len 32, 8 documents (the reference's own CPU-runnable case:
      launch-bound on a GPU; d_model 128 runs on the generic tile kernels, "fused_path": false)
  c2 (default; the configuration the metric is quoted on)  Crello Ours-IMP: masking_method=random,
     d_model 256, 4 blocks, seq_len 128, 256 documents/GPU, bf16 MFMA operands + f32 accumulation
  c3  c2 with masking_method=elem_pos_attr_img_txt (Ours-EXP: all five task types active)
  c4  c2 with 128 documents/GPU (global batch 1024 at --gpus 8)
  c5  Crello Ours-EXP-FT shape: d_model 512, 8 blocks, seq_len 256, 64 documents/GPU, bf16 (default since round 6); the
      line also carries "fp8_mode": the same step with the e4m3 QKV / FFN1 forward products as OCP-MX block-scaled products
      (one e8m0 scale per 32 input features, v_mfma_scale_f32_16x16x128_f8f6f4) -- slower than bf16 and 1.5e-2 off the
      oracle, kept as a precision-only mode (`--dtype fp8` times it alone)

Timed region: K hipGraph replays of the captured step between two device synchronisations (+ barriers for N > 1);
`value` = elements of all ranks / that wall time, `ms_per_step` = that wall time / K; `ms_per_step_median` (`--full`) =
median of the per-step HIP-event intervals of a second pass over the same K steps (SURVEY.md section 8d asks for the
median; an event between two graph launches costs ~5 us of queue time, so the events stay out of the timed region; the
two agree within that).  The loop ROTATES
`--resident` (default 4) input batches that sit in HBM, each with its own capture of the same step: 4 x 136 MB of f32
embeddings do not fit the 256 MB infinity cache, so every step's inputs are read from HBM like a loader-fed run's
(`input_residency` on the line; `--resident 1` = the single re-masked batch of rounds 1-3).

Extra objects on the line (prompt section 4; roofline, cpu_baseline, fp8_mode and the deviations with `--full` only):
  roofline     - the kernel FAMILY with the largest summed duration in a step.  Durations: the tracer's device times
                 (torch.profiler = roctracer) of the step AS TIMED (hipGraph replay), reported raw
                 (`avg_launch_us_traced`, `frac_traced`) and normalised so that the families sum to the timed step
                 (`avg_launch_us`, `frac`: the tracer stretches kernels by a few percent); algorithmic bytes / FLOPs per
                 launch: the library calls of instrumented eager steps of the same workload (ops._timed);
                 `traffic` = PMC HBM bytes per launch of the same family (profiles/r04_pmc_traffic.json, collected by
                 tools/pmc_step.sh over this same command; falls back to the newest profiles/r*_pmc_traffic.json);
                 `encoder_block` = all kernels of the DeepSVG blocks (forward, backward, weight gradients) summed -- the
                 quantity north_star's MFMA-utilisation target is stated on; `step` = whole-step MFMA fraction
                 (17 320 960 algorithmic FLOP per element at c2).
  fused_path   - false when the configuration falls off the document-tile / activation-stationary kernels
                 (d_model != 256 or seq_len != 128) onto the generic tile kernels.
  dp           - N > 1: ranks seen by a real all-reduce on the nccl (= RCCL) backend, the gradient bucket plan
                 (bytes per bucket, carrier dtype) and `params_in_sync` after the timed steps.
  cpu_baseline - the oracle's eager torch-CPU restatement of the same train step (kind "port"; the
                 TensorFlow reference cannot run here) on a bounded sample, host cores.
  bf16_loss_rel_dev - |loss(bf16 path) - loss(f32 path)| / loss(f32 path) on the first timed-size batch
                 (same masks, same dropout streams); the f32 path is parity-tested against the f64
                 oracle to 1e-5 at this shape (tests/test_gpu_model.py).
  bf16_*_vs_f64_oracle - the same deviations against the f64 ORACLE itself on a B = 4 slice of the timed shape (identical
                 inputs / weights / masks, dropout off): what tests/test_gpu_model.py::test_timed_shape_parity_vs_oracle asserts.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flex-dm_amd"))

CONFIGS = {
    "c1": dict(name="RICO", dataset="rico", masking_method="random", D=128, L=2, S=32, B=8, dtype="bf16"),
    "c2": dict(name="Crello Ours-IMP", masking_method="random", D=256, L=4, S=128, B=256, dtype="bf16"),
    "c3": dict(name="Crello Ours-EXP", masking_method="elem_pos_attr_img_txt", D=256, L=4, S=128, B=256, dtype="bf16"),
    "c4": dict(name="Crello Ours-IMP (global batch 1024 at 8 GPUs)", masking_method="random", D=256, L=4, S=128, B=128,
               dtype="bf16"),
    # (round 6: bf16 is c5's default -- the fp8 mode is slower AND outside north_star's tolerance, so it is
    #  a precision-only mode: its step time and deviation are printed beside the bf16 line as "fp8_mode", `--dtype fp8` times it alone)
    "c5": dict(name="Crello Ours-EXP-FT shape", masking_method="elem_pos_attr_img_txt", D=512, L=8, S=256, B=64,
               dtype="bf16"),
}
MFMA_BF16_DENSE_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: ~2.5 PF dense bf16
HBM_PEAK_GBS = 8000.0


def _pmc_file():
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")))
    return files[-1] if files else None


PMC_FILE = _pmc_file()


def train_flops_per_element(D, L, S, U, n_num):
    """3*L*(16 D^2 + 4 S D) + 2*(2*n_num*512*D) + 3*(2*D*U)."""
    return 3 * L * (16 * D * D + 4 * S * D) + 2 * (2 * n_num * 512 * D) + 3 * (2 * D * U)


def block_flops_per_element(D, L, S):
    """The DeepSVG blocks alone (forward + both gradients): 3*L*(16 D^2 + 4 S D)."""
    return 3 * L * (16 * D * D + 4 * S * D)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--dtype", default=None, choices=["bf16", "fp32", "fp8"], help="override the configuration's compute dtype")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--masking_method", default=None, help="override the configuration's task mix")
    ap.add_argument("--batch", type=int, default=None, help="documents per GPU (override)")
    ap.add_argument("--seq", type=int, default=None, help="positions per document (override; 64 = two documents per 128-row "
                    "tile, the shape of real Crello / RICO batches whose sequences are at most 51 positions long)")
    ap.add_argument("--resident", type=int, default=4, help="input batches resident in HBM that the timed loop rotates")
    ap.add_argument("--full", action="store_true", help="also run the checks and extra measurements (median pass, deviations, "
                    "roofline, c5 fp8 mode, CPU baseline); off: only what the headline figure needs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy")
    return ap.parse_args()


def family(kernel_name):
    return kernel_name.split("<")[0].split("(")[0]


# device-kernel name (as the tracer reports it) -> the family name the library calls are booked under (ops._timed)
_KERNEL_FAMILY = (("attn_bwd", "attn_bwd"), ("attn_fwd", "attn_fwd"), ("ce_tile_kernel", "loss_kernels"),
                  ("mse_kernel", "loss_kernels"), ("zero_sums_kernel", "loss_kernels"),
                  ("dgrad_half_kernel", "dgrad_qkv_kernel"), ("gemm_wgt_kernel", "gemm_wgg_kernel"), ("adam_norm_kernel", "adam_kernels"),
                  ("adam_update_kernel", "adam_kernels"), ("transpose_cast_kernel", "cast_kernel"),
                  ("embed_fwd_lds_kernel", "embed_fwd_kernel"), ("embed_onehot_kernel", "embed_fwd_kernel"),
                  ("reduce_rows", "reduce_partials_batch"), ("step_prologue_kernel", "mask_kernel"))


def kernel_family(device_name):
    if "attn_block_fwd_kernel" in device_name:    # <DROPOUT, MLP, STASH, SDOC>: the whole-block variant (MLP) is booked as block_fwd_kernel
        args_ = device_name.split("attn_block_fwd_kernel<")[-1].split(">")[0].replace(" ", "").split(",")
        return "block_fwd_kernel" if len(args_) > 1 and args_[1] in ("true", "1") else "attn_block_fwd_kernel"
    for key, fam in _KERNEL_FAMILY:
        if key in device_name:
            return fam
    n = device_name.replace("void ", "").replace("(anonymous namespace)::", "")
    return family(n)


def replay_kernel_times(model, batch, nrep=3):
    """Per-family device time of the step AS TIMED (hipGraph replay), from the tracer (torch.profiler = roctracer):
    {family: (us per step, launches per step)} and the step's kernel-time total.  The same numbers a
    `rocprofv3 --kernel-trace --stats` of this command gives (profiles/r03_kernel_stats.csv)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    model.train_step(batch)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(nrep):
            model.train_step(batch)
        torch.cuda.synchronize()
    fam = {}
    for e in prof.events():
        if e.device_type.name != "CUDA" or e.device_time_total <= 0:
            continue
        low = e.name.lower()
        if "memcpy" in low or "memset" in low:
            continue
        a = fam.setdefault(kernel_family(e.name), [0.0, 0])
        a[0] += e.device_time_total
        a[1] += 1
    return {k: (v[0] / nrep, v[1] / nrep) for k, v in fam.items()}


def pmc_traffic(fam):
    """(HBM bytes per launch, launches per step) of kernel family `fam` from the L2 memory-side counters
    (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes over this same bench command,
    FETCH_SIZE doubled per the gfx950 correction of MI355X_MICROARCH.md; tools/pmc_step.sh writes the
    file).  Bytes and launches come from the SAME file: one denominator.  None when not collected."""
    try:
        table = json.load(open(PMC_FILE))["kernels"]
    except (OSError, ValueError, KeyError, TypeError):
        return None, None
    tot, calls = 0.0, 0.0
    for k, v in table.items():
        if kernel_family(k) == fam or family(k) == fam:      # (device-kernel name -> the family the library calls are booked under)
            tot += (v["read_mb"] + v["write_mb"]) * 1e6
            calls += v["calls_per_step"]
    return (tot / calls, calls) if calls else (None, None)


def measured_peaks(device):
    """datasheet peaks next to what the box actually delivers -- a hipBLASLt
    bf16 GEMM (torch.matmul, 8192^3) for the matrix pipe and a 1 GiB device copy / fill for HBM."""
    import torch
    out = {}
    a = torch.randn(8192, 8192, device=device, dtype=torch.bfloat16)
    b = torch.randn(8192, 8192, device=device, dtype=torch.bfloat16)
    for _ in range(3):
        torch.matmul(a, b)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        torch.matmul(a, b)
    e1.record(); torch.cuda.synchronize()
    out["hipblaslt_bf16_gemm_8192_tflops"] = 10 * 2 * 8192 ** 3 / (e0.elapsed_time(e1) * 1e-3) / 1e12
    del a, b
    src = torch.empty(1 << 28, device=device, dtype=torch.float32)
    dst = torch.empty_like(src)
    for fn, key, nbytes in ((lambda: dst.copy_(src), "copy_gbs_read_plus_write", 2 * src.numel() * 4),
                            (lambda: dst.fill_(1.0), "fill_gbs_write", src.numel() * 4)):
        for _ in range(2):
            fn()
        e0.record()
        for _ in range(5):
            fn()
        e1.record(); torch.cuda.synchronize()
        out[key] = 5 * nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9
    return out


def _cpu_steps(ic, D, L, S, B, budget_s, min_steps=2, max_steps=200):
    import torch
    from oracle import np_ref, torch_ref
    from mfp.data.spec import synthetic_batch
    params = np_ref.init_params(ic, D, L, seed=0)
    state = torch_ref.TrainState(params, lr=1e-4, l2=1e-2)
    batch = synthetic_batch(ic, B, S, seed=0)
    gen = torch.Generator().manual_seed(0)
    torch_ref.train_step(state, ic, batch, L, rate=0.1, gen=gen, maxlen=S)  # warm-up
    n, t0 = 0, time.time()
    while n < min_steps or (time.time() - t0 < budget_s and n < max_steps):
        torch_ref.train_step(state, ic, batch, L, rate=0.1, gen=gen, maxlen=S)
        n += 1
    dt = time.time() - t0
    return B * S * n / dt, 1e3 * dt / n, n


def cpu_baseline(ic, cfg):
    """Oracle (checker only) timed as the CPU baseline: same train step, eager torch-CPU f32, B = 32 documents per step
    (8 at d_model 512), swept over 1 / 8 / 16 / 32 / all host threads (VERDICT r05 "weak" #9: eager ops this small are slowed
    down by an oversubscribed thread pool, so "all threads" is not the host's best) -- the BEST is quoted as `value`, the sweep
    sits beside it; and config c1, the reference's own CPU-runnable case, at the best thread count.  ~25 s of CPU work."""
    import torch
    from mfp.data.spec import make_input_columns
    D, L, S = cfg["D"], cfg["L"], cfg["S"]
    allthr = torch.get_num_threads()
    B = min(cfg["B"], 32 if D <= 256 else 8)
    counts = sorted({t for t in (1, 8, 16, 32, allthr) if t <= allthr})
    sweep = {}
    try:
        for t in counts:
            torch.set_num_threads(t)
            v, ms, n = _cpu_steps(ic, D, L, S, B, budget_s=max(2.0, 18.0 / len(counts)), min_steps=1)
            sweep[t] = {"value": v, "ms_per_step": ms, "steps": n}
        best = max(sweep, key=lambda t: sweep[t]["value"])
        torch.set_num_threads(best)
        ric = make_input_columns("rico")
        vc, msc, nc = _cpu_steps(ric, 128, 2, 32, 8, budget_s=3.0)
    finally:
        torch.set_num_threads(allthr)
    return {"value": sweep[best]["value"], "unit": "elements/s", "cores": best, "kind": "port", "ms_per_step": sweep[best]["ms_per_step"],
            "sample": "%d train steps of the eager torch-CPU f32 restatement (oracle/torch_ref.py), %s D=%d L=%d S=%d, B=%d "
                      "documents/step (B reduced from %d to bound the sample), dropout 0.1, masking_method=random; best of a "
                      "thread sweep" % (sweep[best]["steps"], cfg.get("dataset", "crello"), D, L, S, B, cfg["B"]),
            "host_threads": allthr,
            "thread_sweep": {str(t): {"value": round(r["value"], 1), "ms_per_step": round(r["ms_per_step"], 1)} for t, r in sweep.items()},
            "c1": {"value": vc, "unit": "elements/s", "cores": best, "ms_per_step": msc,
                   "sample": "%d steps of BASELINE config c1: RICO masking_method=random, 2 blocks, d_model=128, seq_len=32, batch=8" % nc}}


def bf16_deviation(ic, cfg, batch, masking_method, device, dtype="bf16"):
    """Loss of the bf16 (or fp8) path against the f32 (exact-f32 MFMA) path on the same batch, masks and
    dropout streams at step 0 (forward only)."""
    import torch
    from mfp.models.mfp import MFP
    losses = {}
    for dt in ("fp32", dtype):
        m = MFP(ic, num_blocks=cfg["L"], latent_dim=cfg["D"], dropout=0.1, l2=1e-2, masking_method=masking_method,
                dtype=dt, device=device, seed=0)
        m.compile(learning_rate=1e-4, clipnorm=1.0)
        with torch.no_grad():
            _, sums, _ = m._forward(batch)
        m._join_sides()
        torch.cuda.synchronize()
        losses[dt] = sums[:, 0].double().cpu()
        del m
    f, b = losses["fp32"], losses[dtype]
    tot = float(f.sum())
    return {"%s_loss_rel_dev" % dtype: abs(float(b.sum()) - tot) / tot,
            "%s_worst_key_loss_rel_dev" % dtype: float(((b - f).abs() / f.abs().clamp(min=1e-3 * tot)).max())}


def oracle_deviation(ic, cfg, device, dtype="bf16", B=4, mixes=("random",)):
    """Loss of the device path against the f64 ORACLE (checker only, like the cpu_baseline leg) on a B = 4 slice of the timed
    shape: identical inputs, weights and masks (the oracle's masking restatement draws them), dropout off, forward + losses.
    VERDICT r05 "weak" #2: the line used to quote the bf16 path against the f32 DEVICE path, which flatters it."""
    import numpy as np
    import torch
    from oracle import np_masking as om, np_ref, torch_ref
    from mfp.data.spec import synthetic_batch
    from mfp.models.metrics import build_loss_keys, loss_key_names
    from mfp.models.model import Model
    D, L, S = cfg["D"], cfg["L"], cfg["S"]
    nd = {k: v for k, v in ic.items() if not v.get("demo_only")}
    params = np_ref.init_params(ic, D, L, seed=-11)
    batch = synthetic_batch(ic, B, S, seed=31, ragged=True)
    nb = {k: v.numpy() for k, v in batch.items()}
    rng = np.random.default_rng(7)
    draws = {}
    for k, c in nd.items():
        if c["is_sequence"]:
            shp = nb[k].shape
            rnd = rng.integers(0, c["input_dim"], shp) if c["type"] == "categorical" else 0.1 * rng.standard_normal(shp)
            draws[k] = dict(u_mask=rng.random(shp[:2]), u_chg=rng.random(shp[:2]), u_tok=rng.random(shp[:2]), random=rnd)
    _, modified, masks = om.preprocess_for_train(nb, nd, np.zeros(B, np.int32), draws, None, maxlen=S)
    modified.pop("task")
    modified = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in modified.items()}
    masks = {k: torch.from_numpy(v) for k, v in masks.items() if nd[k]["is_sequence"]}
    modified["length"] = batch["length"]
    f64 = lambda d: {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}
    with torch.no_grad():
        p64 = torch_ref.to_torch(params, torch.float64, requires_grad=False)
        total, losses, _, _ = torch_ref.loss_layer(ic, f64(batch), torch_ref.model_fwd(p64, ic, f64(modified), L, maxlen=S), masks, maxlen=S)
    want = float(total)
    model = Model(ic, num_blocks=L, latent_dim=D, dropout=0.0, dtype=dtype, device=device)
    model.store.load_state_dict(params)
    dev = lambda d: {k: v.to(device) for k, v in d.items()}
    keys = build_loss_keys(ic, model.layout.head_cols, dev(batch), dev(masks))
    with torch.no_grad():
        loss, sums, _ = model.forward_loss(dev(modified), keys, training=True)
    torch.cuda.synchronize()
    sums = sums.double().cpu()
    key_rel = {k: abs(float(sums[i, 0]) - float(losses[k])) / max(abs(float(losses[k])), 1e-3 * want) for i, k in enumerate(loss_key_names(ic))}
    worst = max(key_rel, key=key_rel.get)
    return {"%s_loss_rel_dev_vs_f64_oracle" % dtype: abs(float(loss) - want) / want,
            "%s_worst_key_loss_rel_dev_vs_f64_oracle" % dtype: key_rel[worst],
            "%s_worst_key" % dtype: worst,
            "oracle_slice": "B=%d documents (ragged lengths), S=%d, d_model=%d, %d blocks, masking_method=random, dropout 0: identical "
                            "inputs / weights / masks, f64 oracle (oracle/torch_ref.py); a key's loss there is a mean over 9-56 masked "
                            "fields -- attribution of the deviation by rounding site: profiles/r06_bf16_error_budget.txt" % (B, S, D, L)}


DUMP_MAX_BYTES = 48 * 10 ** 6      # (.npy headers aside)


def dump_outputs(out_dir, model, sums, loss):
    """What the last timed step handed its caller, as float32 / float64 .npy files of at most DUMP_MAX_BYTES in all:
      loss_sums - the [nkeys][3] tensor train_step returned (per loss key: loss, score numerator, score denominator)
      loss      - the total loss of the line's final_loss (sum of the per-key losses + the L2 term of the parameters)
      params    - the flat f32 parameter buffer its Adam update left; beyond the byte budget `params_sample` instead: the
                  entries at a fixed sorted index set drawn from numpy's default_rng(0) (the same for every build)"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss_sums": sums.detach().float().cpu().numpy(), "loss": np.array([loss], dtype=np.float64)}
    w = model.model.store.w.detach().float().cpu().numpy()
    room = (DUMP_MAX_BYTES - sum(a.nbytes for a in arrays.values())) // w.itemsize
    if w.size <= room:
        arrays["params"] = w
    else:
        idx = np.sort(np.random.default_rng(0).choice(w.size, room, replace=False))
        arrays["params_sample"] = w[idx]
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world == 1:
        # convenience: relaunch under torchrun exactly as the driver does
        port = os.environ.get("MASTER_PORT", "29511")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    import torch
    import torch.distributed as dist
    from mfp import dp
    from mfp.data.spec import make_input_columns, synthetic_batch
    from mfp.hip import ops
    from mfp.models.mfp import MFP

    cfg = dict(CONFIGS[args.config])
    if args.batch:
        cfg["B"] = args.batch
    if args.seq:
        cfg["S"] = args.seq
    dtype = args.dtype or cfg["dtype"]
    masking_method = args.masking_method or cfg["masking_method"]
    D, NB, S, B = cfg["D"], cfg["L"], cfg["S"], cfg["B"]

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback on the product path)"
    dev_index = local_rank % torch.cuda.device_count()   # (several ranks per GPU only under MFP_DIST_BACKEND=gloo)
    torch.cuda.set_device(dev_index)
    device = "cuda:%d" % dev_index
    world = dp.init_from_env()
    assert world == args.gpus, "WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    torch.manual_seed(1234 + rank)

    ic = make_input_columns(cfg.get("dataset", "crello"))
    batch = synthetic_batch(ic, B, S, seed=rank, ragged=False, device=device)
    roofline = args.full and not args.no_roofline     # (the deviation legs ride with the roofline, as they always did)
    extra = {}
    if roofline and dtype in ("bf16", "fp8") and rank == 0:
        extra = bf16_deviation(ic, cfg, batch, masking_method, device, dtype)
        if cfg.get("dataset", "crello") == "crello":
            try:
                extra.update(oracle_deviation(ic, cfg, device, dtype))
            except Exception as exc:      # a checker leg: never fail the bench line over it
                print("bench.py: oracle deviation unavailable (%s)" % exc, file=sys.stderr)
    model = MFP(ic, num_blocks=NB, latent_dim=D, dropout=0.1, l2=1e-2,
                masking_method=masking_method, dtype=dtype, device=device, seed=0)
    model.compile(learning_rate=1e-4, clipnorm=1.0)
    dp.broadcast_parameters(model.model.store.w)
    model.model.store.refresh_shadow()
    graphed = not args.no_graph
    nres = max(1, args.resident) if world == 1 else 1     # (the N > 1 step is several graphs per step: one buffer set)
    batches = [batch]
    if graphed:
        try:
            model.capture_train_step(batch, warmup=2, resident=nres)
            batch = model.static_batch   # the graph's input buffers: inputs are already resident there
            batches = list(getattr(model, "static_batches", None) or [batch])
            for i, b in enumerate(batches[1:], 1):      # distinct documents in every resident buffer set
                fresh = synthetic_batch(ic, B, S, seed=1000 * i + rank, ragged=False, device=device)
                for k, v in fresh.items():
                    b[k].copy_(v)
        except RuntimeError as e:   # a failed capture must not cost the whole run: step eagerly, say so
            if world == 1:
                raise
            print("bench.py: hipGraph capture failed on rank %d (%s); stepping eagerly" % (rank, e), file=sys.stderr)
            graphed = False
            model._graph = None
            torch.cuda.synchronize()
        if world > 1:   # every rank must step the same way (the graphed path all-reduces in two buckets)
            flag = torch.tensor([1 if graphed else 0], device=device)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if not bool(flag.item()) and graphed:
                graphed = False
                model._graph = None

    def barrier():
        if world > 1:
            dist.barrier()

    if not graphed:
        batches = [batch]
    for i in range(args.warmup):
        model.train_step(batches[i % len(batches)])
    # K steps = K // R replays of the graph that steps through the R resident batches (one graph-launch gap per R steps)
    # + K % R single-step replays
    grouped = graphed and len(batches) > 1 and args.steps >= len(batches) and getattr(model, "train_steps_resident", None) is not None
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if grouped:
        for _ in range(args.steps // len(batches)):
            sums = model.train_steps_resident()
        for i in range(args.steps % len(batches)):      # (K not a multiple of R: the rest as single-step replays)
            sums = model.train_step(batches[i])
    else:
        for i in range(args.steps):
            sums = model.train_step(batches[i % len(batches)])
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    # what the last timed step computed, read before anything else steps the model
    metrics = model.metrics_dict(sums)
    assert metrics["loss"] == metrics["loss"] and abs(metrics["loss"]) < 1e9, "loss is not finite"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, sums, metrics["loss"])
    median_ms = None
    if args.full:
        # the median of per-step intervals: a SECOND pass of the same K steps with an event between consecutive steps (an
        # event record between two graph launches costs ~5 us of queue time per step: not inside the timed region above)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        marks[0].record()
        for i in range(args.steps):
            model.train_step(batches[i % len(batches)])
            marks[i + 1].record()
        torch.cuda.synchronize()
        barrier()
        per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
        median_ms = per_step[len(per_step) // 2] if len(per_step) % 2 else 0.5 * (per_step[len(per_step) // 2 - 1] + per_step[len(per_step) // 2])
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    in_sync = True
    dp_info = None
    if world > 1:   # replicas must hold identical parameters after identical averaged updates
        w = model.model.store.w
        lo, hi = w.clone(), w.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        in_sync = bool(torch.equal(lo, hi)) and bool(torch.isfinite(w).all())
        ones = torch.ones(1, device=device)
        dist.all_reduce(ones)                      # a real collective on the data-path backend: counts the ranks
        dp_info = dp.describe_plan(model.model.layout, graphed)
        launches = getattr(model, "dp_graph_launches_per_step", None) if graphed else None
        dp_info.update({"backend": dist.get_backend(), "collective_ranks": int(ones.item()), "world_size": dist.get_world_size(),
                        "graph_launches_per_step": launches,
                        "graph_mode": ("one graph per step, bucket all-reduces captured inside it" if launches == 1 else
                                       "segments: one graph per backward segment + Adam, eager all-reduces between them")
                        if graphed else "eager"})

    value = world * B * S * args.steps / elapsed
    lay = model.model.layout
    fpe = train_flops_per_element(D, NB, S, lay.U, len(lay.num_keys))
    step_tflops = value / world * fpe / 1e12   # per GPU
    out = {
        "metric": "elements_per_sec_train_step", "value": value, "unit": "elements/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": {"bf16": "bf16", "fp32": "f32", "fp8": "fp8 (MX e4m3 + e8m0 per 32: QKV/FFN1 forward products; bf16 elsewhere)"}[dtype],
        "data": "synthetic",
        "config": {"workload": "%s (%s) train step, masking_method=%s: d_model=%d, %d DeepSVG blocks, seq_len=%d, "
                               "%d documents/GPU, dropout 0.1, l2 1e-2, Adam lr 1e-4 clipnorm 1.0"
                               % (cfg["name"], args.config, masking_method, D, NB, S, B),
                   "dataset": cfg.get("dataset", "crello"),
                   "name": args.config, "global_batch": world * B, "seq_len": S, "parallelism": "dp%d" % world,
                   "launch": ("hipGraph replay, %d steps per graph" % len(batches) if grouped else "hipGraph replay") if graphed else "eager",
                   "params": lay.numel, "train_flop_per_element": fpe},
        "final_loss": metrics["loss"],
        "params_in_sync": in_sync,
        "input_residency": ("%d batches resident in HBM, rotated (%.0f MB of inputs per batch: beyond the 256 MB infinity cache)"
                            % (len(batches), sum(v.numel() * v.element_size() for v in batch.values()) / 1e6)
                            if len(batches) > 1 else "one batch, re-masked every step (its inputs can sit in the infinity cache)"),
        "fused_path": bool((dtype in ("bf16", "fp8") and D == 256 and (S == 128 or (S == 64 and B % 2 == 0))) or (dtype == "bf16" and D == 512)),
    }
    if median_ms is not None:
        out["ms_per_step_median"] = median_ms
    if dp_info is not None:
        out["dp"] = dp_info
    out.update(extra)

    # ---------------- roofline of the dominant kernel family.  Durations: the tracer's device times of the step as
    # timed (hipGraph replay); algorithmic bytes / FLOPs and the block / non-block split of each family: the library
    # calls of instrumented eager steps of the same workload (HIP events on the launch stream; the fallback for the
    # durations when the tracer is unavailable)
    eager_recs, replay = None, None
    if roofline and rank == 0 and graphed and world == 1:
        try:
            replay = replay_kernel_times(model, batch)
        except Exception as exc:   # measurement aid: never fail the bench line over it
            print("bench.py: tracer unavailable (%s); event-timed eager durations" % exc, file=sys.stderr)
    if roofline:
        # instrumented eager steps (HIP events around the library calls): EVERY rank steps -- with N > 1 an eager step
        # all-reduces the gradients, so rank 0 alone would wait for its peers forever -- rank 0 reports
        model._graph = None
        model.train_step(batches[0])
        torch.cuda.synchronize()
        ops.start_profile()
        for _ in range(3):
            model.train_step(batches[0])
        eager_recs = (ops.stop_profile(), 3)
        barrier()
    if roofline and rank == 0:
        recs, nprof = eager_recs
        agg, blk, blk_ms = {}, [0.0, 0.0, 0.0], {}
        for name, flops, nbytes, ms, scope, share in recs:      # share < 1: one launch booked under several scopes
            a = agg.setdefault(family(name), [0, 0.0, 0.0, 0.0])
            a[0] += share; a[1] += flops; a[2] += nbytes; a[3] += ms
            if scope == "block":
                blk[0] += flops; blk[1] += nbytes; blk[2] += ms
                blk_ms[family(name)] = blk_ms.get(family(name), 0.0) + ms
        blk_share_den = {k: a[3] for k, a in agg.items()}      # (eager event time per family: the denominator of its block share)
        timing = "HIP events around the library calls of eager steps"
        missing = [k for k in agg if replay is None or k not in replay]
        if replay is not None and missing:
            print("bench.py: families without traced kernels: %s (replay saw %s)" % (missing, sorted(replay)), file=sys.stderr)
        if replay is not None and not missing:
            # replay durations per family; a family's block share = its share in the eager records (same launches).
            # The tracer stretches every kernel a little (its durations sum to ~6 % more than the timed step although
            # the replayed kernels run back to back: profiles/r03_step_dump.txt): normalised to the timed step.
            traced = sum(v[0] for v in replay.values())
            norm = min(1.0, out["ms_per_step"] * 1e3 / traced)
            out["tracer_normalisation"] = norm
            blk[2] = sum(replay[k][0] * norm * 1e-3 * nprof * blk_ms.get(k, 0.0) / agg[k][3] for k in agg if agg[k][3] > 0)
            for k in agg:
                agg[k][3] = replay[k][0] * norm * 1e-3 * nprof
            timing = ("tracer device times of the hipGraph-replayed step (torch.profiler / roctracer), normalised so that "
                      "they sum to the timed step (kernels run back to back under replay)")
            out["replay_traced_kernel_us_per_step"] = round(traced, 1)
        total_ms = sum(a[3] for a in agg.values())
        table = sorted(agg.items(), key=lambda kv: -kv[1][3])
        name, (cnt, flops, nbytes, ms) = table[0]
        # the encoder block (its products, attention, their gradients) is priced against the MFMA roof
        # -- the block forward is NOT HBM-bound -- and the streaming kernels (gather / pool, LayerNorm, loss,
        # masking, optimizer) against the HBM roof.  A family is a block family when most of its time is booked under the
        # "block" scope of the instrumented steps.  Both fractions are printed for every family (`families`).
        def fam_row(k, v):
            c_, fl_, by_, ms_ = v
            tf_, gb_ = fl_ / (ms_ * 1e-3) / 1e12, by_ / (ms_ * 1e-3) / 1e9
            pm, _ = pmc_traffic(k) if args.config == "c2" and dtype == "bf16" else (None, None)
            return {"us_per_step": round(1e3 * ms_ / nprof, 1), "launches_per_step": round(c_ / nprof, 2),
                    "bound": "mfma" if fl_ > 0 and blk_ms.get(k, 0.0) >= 0.5 * blk_share_den[k] else "hbm",
                    "mfma_frac": round(tf_ / MFMA_BF16_DENSE_PEAK_TFLOPS, 4), "hbm_frac": round(gb_ / HBM_PEAK_GBS, 4),
                    "algorithmic_mb_per_launch": round(by_ / c_ / 1e6, 2), "pmc_mb_per_launch": None if pm is None else round(pm / 1e6, 2)}
        families = {k: fam_row(k, v) for k, v in table if v[3] > 0 and v[0] > 0}
        tf = flops / (ms * 1e-3) / 1e12
        gbs = nbytes / (ms * 1e-3) / 1e9
        f_mfma, f_hbm = tf / MFMA_BF16_DENSE_PEAK_TFLOPS, gbs / HBM_PEAK_GBS
        if families[name]["bound"] == "hbm":
            roof = {"bound": "hbm", "kernel": name, "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": f_hbm, "mfma_frac": f_mfma}
        else:
            roof = {"bound": "mfma", "kernel": name, "achieved": tf, "peak": MFMA_BF16_DENSE_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": f_mfma, "hbm_frac": f_hbm}
        # the family furthest below ITS roof among those that cost >= 3 % of the step
        far = min((k for k in families if families[k]["us_per_step"] >= 0.03 * 1e3 * total_ms / nprof),
                  key=lambda k: families[k]["mfma_frac" if families[k]["bound"] == "mfma" else "hbm_frac"], default=None)
        roof["families"] = families
        roof["furthest_from_roof"] = far
        roof["algorithmic_bytes_per_launch"] = nbytes / cnt
        if "tracer_normalisation" in out:      # the same fraction from the tracer's raw durations
            roof["frac_traced"] = roof["frac"] * out["tracer_normalisation"]
            roof["avg_launch_us_traced"] = 1e3 * ms / cnt / out["tracer_normalisation"]
        roof["launches_per_step"] = cnt / nprof
        traffic, pmc_calls = pmc_traffic(name) if args.config == "c2" and dtype == "bf16" else (None, None)
        roof["traffic"] = traffic
        if traffic is not None:
            # PMC counters cannot be read from inside the process: the bytes come from the committed rocprofv3 --pmc passes
            # over this same command (tools/pmc_step.sh), not from this run
            roof["traffic_source"] = os.path.relpath(PMC_FILE, ROOT)
            roof["traffic_launches_per_step"] = pmc_calls   # must equal launches_per_step (same command)
        block_fl = block_flops_per_element(D, NB, S) * B * S
        roof.update({"avg_launch_us": 1e3 * ms / cnt, "timing": timing,
                     "share_of_instrumented_kernel_time": ms / total_ms,
                     "encoder_block": {
                         "us_per_step": 1e3 * blk[2] / nprof,
                         "mfma_frac": (block_fl / (blk[2] / nprof * 1e-3) / 1e12) / MFMA_BF16_DENSE_PEAK_TFLOPS,
                         "achieved_tflops": block_fl / (blk[2] / nprof * 1e-3) / 1e12,
                         "hbm_frac": (blk[1] / nprof / (blk[2] / nprof * 1e-3) / 1e9) / HBM_PEAK_GBS,
                         "algorithmic_gb_per_step": blk[1] / nprof / 1e9,
                         "note": "all kernels of the DeepSVG blocks (LN, QKV/O/FFN GEMMs, attention, their input and "
                                 "weight gradients), all on one stream; durations: " + timing},
                     "step": {"achieved": step_tflops, "peak": MFMA_BF16_DENSE_PEAK_TFLOPS, "unit": "TFLOP/s",
                              "frac": step_tflops / MFMA_BF16_DENSE_PEAK_TFLOPS},
                     "kernels_us_per_step": {k: round(1e3 * v[3] / nprof, 1) for k, v in table}})
        try:
            mp = measured_peaks(device)
            roof["measured_peaks"] = mp
            roof["frac_of_measured_peak"] = (roof["achieved"] / mp["copy_gbs_read_plus_write"] if roof["bound"] == "hbm"
                                             else roof["achieved"] / mp["hipblaslt_bf16_gemm_8192_tflops"])
            roof["step"]["frac_of_measured_gemm_peak"] = step_tflops / mp["hipblaslt_bf16_gemm_8192_tflops"]
        except Exception as exc:   # measurement aid only: never fail the bench line over it
            roof["measured_peaks"] = "unavailable: %s" % exc
        out["roofline"] = roof
    if roofline and args.config == "c5" and dtype == "bf16" and world == 1:
        # BASELINE config 5 names fp8: the precision-only mode's figures beside the bf16 line (same command, --dtype fp8)
        try:
            del model
            torch.cuda.empty_cache()
            cmd = [sys.executable, os.path.abspath(__file__), "--config", "c5", "--dtype", "fp8", "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--no-cpu-baseline", "--no-roofline"]
            f8 = json.loads(subprocess.run(cmd, capture_output=True, text=True, timeout=900).stdout.strip().splitlines()[-1])
            out["fp8_mode"] = {"ms_per_step": f8["ms_per_step"], "value": f8["value"], "unit": "elements/s",
                               "vs_bf16": out["ms_per_step"] / f8["ms_per_step"],
                               "loss_rel_dev_vs_f64_oracle_at_B2": 1.49e-2,
                               "note": "precision-only mode (DESIGN.md section 4): MX e4m3 Q|K|V / FFN1 forward products, bf16 elsewhere; "
                                       "the deviation (tests/test_gpu_model.py::test_c5_shape_parity_vs_oracle[fp8]) is carried by the "
                                       "e4m3 WEIGHT rounding and is outside north_star's 1e-3"}
        except Exception as exc:
            out["fp8_mode"] = "unavailable: %s" % exc
    if args.full and not args.no_cpu_baseline and rank == 0 and world == 1:
        out["cpu_baseline"] = cpu_baseline(ic, cfg)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
