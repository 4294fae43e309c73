"""Headline benchmark: training images/sec (fwd + bwd + SGD step) of BCNN
(VGG-16, 448x448, C=512, 200 classes, batch 64 per GPU) - BASELINE.json's metric on
BASELINE.json configs[1] (`BCNN_S2.yaml on 1xMI355X`).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W
(the first form with N > 1 starts the second one as a child: one process per GPU over RCCL)

One step = one minibatch already resident in HBM -> model forward (VGG-16 on
MIOpen, bilinear pooling on the gfx950 kernels) -> CrossEntropy(label_smoothing
0.1) -> backward -> SGD(momentum 0.9) step.  fp32
throughout (the reference's dtype; parity target 1e-4).  Weak scaling: every
rank trains batch 64; `value` = all images of all ranks / max-over-ranks time.

Rank 0 prints ONE short JSON line as the LAST line of stdout (< 4 KB: `final_line`).  A plain run does only what that
line's headline needs: set up, warm up, time --steps steps, write the last step's outputs (--dump-outputs DIR), print.
  --dump-outputs DIR  after the timed steps: DIR/<name>.npy (float32) of what the last timed step computed - the loss, the
                      model's outputs and a fixed, seeded sample of every updated parameter (< 64 MB in all); the inputs
                      are seeded, so two builds run with the same arguments can be compared output for output
  --full              also measure everything beyond the headline.  At N=1 the line then carries
    roofline     - the dominant hand-written kernel of the step: algorithmic FLOPs / HIP-event time
    cpu_baseline - the oracle's BCNN (reference algorithm on the torch CPU path) timed on the host cores
  and everything else (per-kernel rows of the pooling head, the other BASELINE.json configs, the hipGraph rows, the DDP
  bucket timeline) goes to the detail file (`emit`: $HAWKEYE_BENCH_DETAIL, else its default path) and, as a short table,
  to stderr - never onto the line the driver parses.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hawkeye_amd.miopen_cache import use_in_tree_cache  # noqa: E402

use_in_tree_cache()       # MIOpen JIT cache inside the repo (no gfx950 kernel db in the image): see miopen_cache.py

PEAK_MFMA_F32_TF = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_HBM_GBS = 8000.0         # HBM3E spec (6.3 TB/s achievable)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64, help='per-GPU batch (metric: 64)')
    ap.add_argument('--image', type=int, default=448)
    ap.add_argument('--classes', type=int, default=200)
    ap.add_argument('--model', default='BCNN', choices=['BCNN', 'CBCNN', 'MPN', 'APCNN', 'OSMENet', 'CIN'],
                    help='BCNN is the metric; the others are side measurements (OSMENet / CIN: --image 224, their own criteria)')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-kernels', action='store_true')
    ap.add_argument('--channels-last', type=int, default=1,
                    help='NHWC tensors through the backbone: MIOpen picks NHWC igemm kernels either way; this removes its '
                         'NCHW<->NHWC batched_transpose passes (5.7%% of the step): measured 298.8 vs 273.2 img/s')
    ap.add_argument('--miopen-find', type=int, default=0)
    ap.add_argument('--verbose', action='store_true')
    ap.add_argument('--backend', default=None, help='process-group backend override (debug: gloo lets N ranks share one GPU)')
    ap.add_argument('--share-gpu', action='store_true', help='debug: every rank uses cuda:0')
    ap.add_argument('--force-pg', action='store_true',
                    help='create the process group even for one rank: the bucketed RCCL all-reduce path then executes on a '
                         'one-GPU box (adds `ddp_timeline` to the JSON line)')
    ap.add_argument('--ddp-trace', action='store_true', help='N > 1: add `ddp_timeline` (where in the backward each '
                                                             'gradient bucket\'s all-reduce was issued)')
    ap.add_argument('--kernels-first', action='store_true',
                    help='--full: also time the pooling-head kernels BEFORE the training loop (`kernels_before`): the same '
                         'kernels read 1.2-1.4x slower right after 25 conv-bound steps (power-limited clocks) than on a cool chip')
    ap.add_argument('--no-other-models', action='store_true',
                    help='skip the subprocess that times the other BASELINE.json configs (MPN, CBCNN, APCNN-8142)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline, also measure what it does not need: per-kernel rooflines, the CPU baseline, the '
                         'other configs, the hipGraph rows, the DDP bucket timeline (the --no-* options above trim this)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write what the last timed step computed to DIR/<name>.npy (float32)')
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    return a


def free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def host_threads_per_rank(world):
    return max(1, min(32, (os.cpu_count() or 1) // max(world, 1)))


def device_identity(dev):
    """What tells two GPUs apart on one node: PCI domain:bus:device and the uuid (torch's device properties)."""
    p = torch.cuda.get_device_properties(dev)
    pci = ':'.join(f'{getattr(p, k):x}' for k in ('pci_domain_id', 'pci_bus_id', 'pci_device_id') if hasattr(p, k))
    return {'index': dev.index, 'pci': pci or None, 'uuid': str(getattr(p, 'uuid', '')) or None, 'name': p.name}


def gather_rank_devices(rank, world, dev):
    """N > 1: every rank's host pid and device identity, gathered to all ranks - the first multi-GPU run then says by
    itself whether N ranks really sat on N different GPUs (`distinct_devices` == N unless --share-gpu)."""
    me = dict(rank=rank, pid=os.getpid(), **device_identity(dev))
    seen = [None] * world
    torch.distributed.all_gather_object(seen, me)
    ids = {(d['pci'], d['uuid']) if (d['pci'] or d['uuid']) else ('index', d['index']) for d in seen}
    return {'ranks_seen': sorted(d['rank'] for d in seen), 'distinct_devices': len(ids),
            'devices': [d['pci'] or d['uuid'] or str(d['index']) for d in sorted(seen, key=lambda d: d['rank'])]}


def respawn_one_rank_per_gpu(a):
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: run
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <same arguments>` as a child (one process
    per GPU; rank 0 prints the JSON line) and exit with its status.  A child, not an exec: this process has already asked
    the runtime for the device count.  Replaces train.py:220-228's single-process nn.DataParallel."""
    if not a.share_gpu and torch.cuda.device_count() < a.gpus:
        sys.exit(f'bench.py: --gpus {a.gpus} but only {torch.cuda.device_count()} GPU(s) visible '
                 f'(--share-gpu --backend gloo runs the ranks on one GPU for a functional check)')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={a.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    # host threads: N ranks x (all cores) OpenMP threads oversubscribe the host (the optimiser's foreach kernels and the
    # pinned-memory copies run on them); give each rank its share before torch is imported in the children
    env.setdefault('OMP_NUM_THREADS', str(host_threads_per_rank(a.gpus)))
    import subprocess
    sys.stdout.flush()
    rc = subprocess.run(cmd, env=env).returncode
    sys.exit(rc if rc >= 0 else 128 - rc)            # killed by a signal: the shell's 128 + signal


def build_model(name, classes):
    import hawkeye_amd.model  # noqa: F401
    from hawkeye_amd.config import CfgNode
    from hawkeye_amd.model.registry import MODEL
    cfgs = {
        'BCNN': dict(name='BCNN', stage=2, num_classes=classes),
        'CBCNN': dict(name='CBCNN', stage=2, num_classes=classes, input_channel=512, output_channel=6000),
        'MPN': dict(name='MPN', iter_num=5, is_sqrt=True, is_vec=True, input_dim=2048, dimension_reduction=256,
                    num_classes=classes),
        'APCNN': dict(name='APCNN', num_classes=classes),
        'OSMENet': dict(name='OSMENet', num_attention=2, num_classes=classes),
        'CIN': dict(name='CIN', num_classes=classes),
    }
    cfg = CfgNode(cfgs[name])
    cfg.freeze()
    return MODEL.get(name)(cfg)


def time_events(fn, iters, warm=3, rounds=1):
    """Average duration (ms) of fn() measured with HIP events on torch's current stream - the stream the
    C ABI launches on (functional.stream()).  rounds > 1: that many back-to-back rounds of `iters` launches with no
    host synchronisation in between; returns (last round, first round).  Under a sustained fp32-MFMA load the chip's
    clock settles only after ~10 ms (tools/bwd_ab.py: 77 -> 72 -> 69.5 us over the first three rounds of the same
    kernel), so a kernel timed cold is 8-10 % slower than the same kernel inside a busy training step."""
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(rounds + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for r in range(rounds):
        for _ in range(iters):
            fn()
        ev[r + 1].record()
    torch.cuda.synchronize()
    if rounds == 1:
        return ev[0].elapsed_time(ev[1]) / iters
    return ev[rounds - 1].elapsed_time(ev[rounds]) / iters, ev[0].elapsed_time(ev[1]) / iters


def roof_row(name, us, flops_alg, bytes_alg, flops_exec=None, us_first=None):
    """One roofline row.  `flops_alg` / `bytes_alg` are the ALGORITHMIC work per launch;
    `flops_exec` what the kernel really issues to the matrix pipe when that differs (the symmetric Gram forward computes
    36 of 64 tiles, the classifier pads 200 classes to 208).  `frac` is priced on min(algorithmic, executed): a kernel
    that skips work the algorithm does not need is not credited with it, a kernel that pads is not credited with the
    padding - so frac <= the busy fraction of the pipe and never exceeds 1."""
    fe = flops_alg if flops_exec is None else flops_exec
    fl = min(flops_alg, fe)
    bound = 'mfma' if fl > 0 and flops_alg / max(bytes_alg, 1.0) > PEAK_MFMA_F32_TF * 1e3 / PEAK_HBM_GBS else 'hbm'
    tf, gbs = fl / us / 1e6, bytes_alg / us / 1e3
    row = {'kernel': name, 'us': round(us, 2), 'bound': bound,
           'achieved': round(tf if bound == 'mfma' else gbs, 2),
           'peak': PEAK_MFMA_F32_TF if bound == 'mfma' else PEAK_HBM_GBS,
           'unit': 'TFLOP/s' if bound == 'mfma' else 'GB/s',
           'frac': round(min((tf / PEAK_MFMA_F32_TF) if bound == 'mfma' else (gbs / PEAK_HBM_GBS), 1.0), 4),
           'traffic': None, 'flops_algorithmic': flops_alg, 'flops_executed': fe, 'bytes_algorithmic': bytes_alg}
    if bound == 'mfma':
        row['frac_hbm'] = round(gbs / PEAK_HBM_GBS, 4)
    if us_first is not None:
        row['us_first_round'] = round(us_first, 2)
    return row


def kernel_rooflines(B, C, HW, dev):
    """Per-stage timing of the bilinear-pooling head + classifier at the metric's shape.  Algorithmic work:
    gram_norm  FLOPs 2*B*C*C*HW ; bytes 4*B*C*HW (x) + 4*B*C*C (y)
    bwd_gemm   FLOPs 2*B*C*C*HW ; bytes 2*4*B*C*C (y, dy) + 2*4*B*C*HW (x, dx)
    colsum     bytes 4*B*C*HW ;  rank1 bytes 2*4*B*C*HW
    classifier fwd FLOPs 2*B*J*K ; bytes 4*(K*J + B*J + B*K);  bwd twice that (dy = g W and dW = g^T y)"""
    from hawkeye_amd import _lib
    from hawkeye_amd._lib import ptr, stream
    lib = _lib.load()
    x = torch.relu(torch.randn(B, C, HW, device=dev))
    y = torch.empty(B, C * C, device=dev)
    dy = torch.randn(B, C * C, device=dev)
    dx = torch.empty_like(x)
    inv = torch.empty(B, device=dev)
    cs = torch.empty(B, HW, device=dev)
    tp = torch.empty(B, (C + 63) // 64, device=dev)
    nwsc = lib.hk_bcnn_pool_ws_bytes(B, C, HW)
    wsc = torch.empty(nwsc, dtype=torch.uint8, device=dev)
    lib.hk_bcnn_colsum_norm(ptr(x), ptr(cs), ptr(inv), B, C, HW, ptr(wsc), nwsc, stream())
    lib.hk_bcnn_gram_norm(ptr(x), ptr(inv), ptr(y), B, C, HW, stream())
    flops = 2.0 * B * C * C * HW
    nb = C // 64
    sym = (nb * (nb + 1) // 2) / float(nb * nb) if C % 64 == 0 else 1.0      # tiles J >= I only
    K, J = 200, C * C
    wl, bl = torch.randn(K, J, device=dev) * 0.01, torch.zeros(K, device=dev)
    ol, gl = torch.empty(B, K, device=dev), torch.randn(B, K, device=dev)
    dyl, dwl, dbl = torch.empty(B, J, device=dev), torch.empty(K, J, device=dev), torch.empty(K, device=dev)
    nwl = lib.hk_linear_ws_bytes(B, J, K)
    wsl = torch.empty(nwl, dtype=torch.uint8, device=dev)
    lflops, lbytes = 2.0 * B * J * K, 4.0 * (K * J + B * J + B * K)
    kpad = (K + 15) // 16 * 16 / float(K)
    # the backward's kernel by the library's own dispatch rule (bcnn_fast.hip bwd_launch: 128-row blocks when they fill
    # the chip, else 64-row blocks, else the four-wave panel kernel; the generic tiles outside the fast shapes)
    if C % 64 == 0 and HW in (196, 144, 100, 64):
        rb = 2 if (C % 128 == 0 and B * (C // 128) >= 192) else (1 if B * nb >= 192 else 0)
        bwd_name = f'gram_bwd3_kernel<{HW},0,{rb}>' if rb else f'bcnn_bwd_panel_kernel<{HW},0>'
    else:
        bwd_name = 'bgemm_kernel (generic tiles: not a fast shape)'
    gram_name = f'bcnn_gram_panel_kernel<{HW}>' if C % 64 == 0 and HW in (196, 144, 100, 64) else 'bgemm_kernel (generic tiles)'
    stages = [
        ('bcnn_colsum_partial4_kernel + finalize (stage entry point)',
         lambda: lib.hk_bcnn_colsum_norm(ptr(x), ptr(cs), ptr(inv), B, C, HW, ptr(wsc), nwsc, stream()),
         0.0, 4.0 * B * C * HW, None, False),
        ('hk_bcnn_pool_fwd, whole (ONE launch: the Gram kernel adds up the sample\'s columns in its prologue)',
         lambda: lib.hk_bcnn_pool_fwd(ptr(x), ptr(y), ptr(inv), ptr(cs), B, C, HW, ptr(wsc), nwsc, stream()),
         flops, 8.0 * B * C * HW + 4.0 * B * C * C, flops * sym, False),
        (gram_name, lambda: lib.hk_bcnn_gram_norm(ptr(x), ptr(inv), ptr(y), B, C, HW, stream()),
         flops, 4.0 * B * C * HW + 4.0 * B * C * C, flops * sym, True),
        (bwd_name,
         lambda: lib.hk_bcnn_bwd_gemm(ptr(x), ptr(y), ptr(dy), ptr(inv), ptr(dx), ptr(tp), B, C, HW, stream()),
         flops, 8.0 * B * C * C + 8.0 * B * C * HW, None, True),
        ('bcnn_rank1_fix_kernel', lambda: lib.hk_bcnn_bwd_rank1(ptr(dx), ptr(tp), ptr(inv), ptr(cs), B, C, HW, stream()),
         0.0, 8.0 * B * C * HW, None, True),
        ('hk_bcnn_pool_bwd, whole (two launches: GEMM kernel + rank-1 pass; dy from anywhere)',
         lambda: lib.hk_bcnn_pool_bwd(ptr(x), ptr(y), ptr(dy), ptr(inv), ptr(cs), ptr(dx), B, C, HW, ptr(wsc), nwsc, stream()),
         flops, 8.0 * B * C * C + 8.0 * B * C * HW, None, False),
        ('hk_bcnn_pool_bwd_tdot, whole (ONE launch: <y, dy> from the classifier, rank-1 term in the GEMM epilogue; what BCNN runs)',
         lambda: lib.hk_bcnn_pool_bwd_tdot(ptr(x), ptr(y), ptr(dy), ptr(inv), ptr(cs), ptr(gl), ptr(ol), ptr(bl), K, ptr(dx), B, C, HW,
                                           ptr(wsc), nwsc, stream()),
         flops, 8.0 * B * C * C + 8.0 * B * C * HW, None, False),
        ('hk_linear_fwd: linear_skinny_kernel + linear_reduce_kernel (classifier 262144->200)',
         lambda: lib.hk_linear_fwd(ptr(y), ptr(wl), ptr(bl), ptr(ol), B, J, K, ptr(wsl), nwl, stream()),
         lflops, lbytes, lflops * kpad, True),
        ('hk_linear_bwd: linear_bwd64_kernel (dy = g W, dW = g^T y, db in one launch; classifier 262144->200)',
         lambda: lib.hk_linear_bwd(ptr(y), ptr(wl), ptr(gl), ptr(dyl), ptr(dwl), ptr(dbl), B, J, K, stream()),
         2 * lflops, 2 * lbytes, lflops * (1.0 + kpad), True),
    ]
    out = []
    for name, fn, fl, by, fe, single in stages:
        ms, ms_first = time_events(fn, 50, rounds=4)       # steady state: the fourth back-to-back round of 50 launches
        row = roof_row(name, ms * 1e3, fl, by, fe, ms_first * 1e3)
        row['shipped_kernel'] = single      # False: a stage entry point / a multi-launch sum, not a candidate for `roofline`
        out.append(row)
    return out


def pmc_traffic(row_name):
    """HBM bytes per launch sequence of a `kernel_rooflines` row from the committed rocprofv3 PMC passes
    (profiles/rN_pool_kernels_pmc.csv: FETCH_SIZE / WRITE_SIZE in KiB, separate --pmc passes; FETCH_SIZE doubled - gfx950
    reports half of the bytes of 16-B-per-lane streaming reads, MI355X_MICROARCH.md section HBM), summed over every
    kernel the row names.  PMC cannot be sampled from inside this process, so this is the last profiled value, or None
    when no file has all of the row's kernels."""
    import csv
    import re
    names = re.findall(r'[a-z][a-z0-9_]*_kernel', row_name)
    for name in ('r6_step_BCNN_pmc.csv', 'r5_pool_kernels_pmc.csv', 'r4_pool_kernels_pmc.csv'):    # newest first (r6: counted INSIDE the step)
        try:
            rows = list(csv.DictReader(open(os.path.join(ROOT, 'profiles', name))))
            total = 0.0
            for kn in names:
                vals = {r['Counter']: float(r['MeanValue']) for r in rows
                        if r['Kernel'].replace('void ', '').startswith('hk::' + kn) and r['Counter'] in ('FETCH_SIZE', 'WRITE_SIZE')}
                total += (2.0 * vals['FETCH_SIZE'] + vals['WRITE_SIZE']) * 1024.0
            if names:
                return round(total), 'profiles/' + name
        except Exception:  # noqa: BLE001
            continue
    return None, None


def cpu_baseline(image, classes):
    """Reference algorithm on the host: the oracle's BCNN (VGG-16 + BilinearPooling on the torch CPU path, i.e. what
    the reference executes with `experiment.cuda: []`) training step at batch 4 (BASELINE.json configs[0]).
    Bounded: 1 warm-up + at most 3 timed steps or ~25 s.  Threads: min(host cores, 32) - oneDNN convolutions at
    batch 4 stop scaling (and on a 256-core host get much slower) beyond that; `cores` reports what was used."""
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import hawkeye_oracle as O
    threads = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    bs = 4
    m = O.BCNNOracle(classes, stage=2)
    opt = torch.optim.SGD(m.parameters(), lr=0.005, momentum=0.9, weight_decay=1e-5)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    x = torch.randn(bs, 3, image, image)
    y = torch.randint(0, classes, (bs,))
    times = []
    for it in range(4):
        t0 = time.time()
        loss = crit(m(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        dt = time.time() - t0
        if it > 0:
            times.append(dt)
        if it > 0 and sum(times) > 25:
            break
    best = min(times)
    return {'value': round(bs / best, 3), 'unit': 'images/sec', 'cores': threads, 'kind': 'port',
            'sample': f'BCNN stage-2 train step, batch {bs}, {image}x{image}, best of {len(times)} after 1 warm-up, '
                      f'torch CPU fp32, {threads} threads of {os.cpu_count()} host cores'}


def other_models(timeout_s=240):
    """The other BASELINE.json configs on this GPU (configs[2..4] at their single-GPU shapes): MPN bs64, CBCNN bs64 /
    bs16, AP-CNN with the iNat2018 class count (8142) bs16 - ms/step, images/sec and the per-kernel rooflines of their
    pooling heads (tools/model_rows.py).  Subprocess after the headline, like `candidates`: cannot touch `value`."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'model_rows.py')]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {'error': f'timeout after {timeout_s}s'}
    except Exception as e:  # noqa: BLE001
        return {'error': repr(e)[:300]}
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('[')]
    if p.returncode != 0 or not lines:
        return {'error': f'rc={p.returncode}', 'stderr_tail': p.stderr[-400:]}
    try:
        return json.loads(lines[-1])
    except ValueError as e:
        return {'error': repr(e)[:300]}


def graph_rows(timeout_s=200):
    """Every pooling head, forward + backward, captured in a hipGraph and replayed (tools/graph_rows.py): bit identity with
    the eager run and eager-vs-replay time per head.  Subprocess after the headline; detail file only."""
    import subprocess
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'graph_rows.py'), '--quick'], capture_output=True, text=True,
                           cwd=ROOT, timeout=timeout_s)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('[')]
        return json.loads(lines[-1]) if p.returncode == 0 and lines else {'error': f'rc={p.returncode}', 'stderr_tail': p.stderr[-300:]}
    except Exception as e:  # noqa: BLE001
        return {'error': repr(e)[:300]}


DUMP_MAX_BYTES = 64 << 20


def output_tensors(obj, name='output'):
    """(name, tensor) for every tensor in a model's output: a tensor, or tuples / lists / dicts of them."""
    if torch.is_tensor(obj):
        return [(name, obj)]
    if isinstance(obj, dict):
        return [r for k, v in obj.items() for r in output_tensors(v, f'{name}.{k}')]
    if isinstance(obj, (list, tuple)):
        return [r for i, v in enumerate(obj) for r in output_tensors(v, f'{name}.{i}')]
    return []


def dump_outputs(path, loss, out, model):
    """What the last timed step computed, as DIR/<name>.npy in float32: `loss`, `output[.i...]` (the model's outputs) and
    `param.<name>` (every parameter after the optimiser step).  An array larger than `cap` elements is replaced by a fixed,
    seeded sample of `cap` of its elements (the same indices in every run), so the files stay under DUMP_MAX_BYTES."""
    import numpy as np
    arrays = [('loss', loss.detach().reshape(1))] + [(n, t.detach()) for n, t in output_tensors(out)] + \
             [('param.' + n, p.detach()) for n, p in model.named_parameters()]
    cap = max(1024, min(1 << 20, DUMP_MAX_BYTES // 4 // len(arrays)))
    os.makedirs(path, exist_ok=True)
    total = 0
    for i, (name, t) in enumerate(arrays):
        if t.numel() > cap:
            idx = torch.randint(0, t.numel(), (cap,), generator=torch.Generator().manual_seed(i)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        a = np.ascontiguousarray(t.float().cpu().numpy(), dtype=np.float32)
        total += a.nbytes
        assert total <= DUMP_MAX_BYTES, (name, total)
        np.save(os.path.join(path, name + '.npy'), a)
    return total


LINE_KEYS = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
             'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'ddp')
LINE_MAX = 4096


def final_line(res):
    """The one line the driver parses: the contract's keys + `roofline` + `cpu_baseline`, nothing else, < 4 KB
    (round 3's 24.5 KB line - 84 A/B rows on it - was past the driver's capture window: BENCH_r03.json parsed: null).
    tests/test_bench_line_cpu.py holds this to the limit on canned numbers."""
    line = json.dumps({k: res[k] for k in LINE_KEYS if k in res}, separators=(',', ':'))
    if len(line) >= LINE_MAX:                             # never lose the headline to an oversized field
        slim = {k: res[k] for k in LINE_KEYS if k in res}
        for k in ('cpu_baseline', 'roofline'):
            if isinstance(slim.get(k), dict):
                slim[k] = {kk: (vv[:80] if isinstance(vv, str) else vv) for kk, vv in slim[k].items()}
        line = json.dumps(slim, separators=(',', ':'))
    assert len(line) < LINE_MAX and '\n' not in line, len(line)
    return line


def emit(res, detail, seal=False):
    """Detail -> gpurun_out/bench_detail.json + a short table on stderr; then the final line, last on stdout."""
    if detail:
        # (HAWKEYE_BENCH_DETAIL: where the tests' own bench runs put theirs - not over the record of the real one)
        path = os.environ.get('HAWKEYE_BENCH_DETAIL') or os.path.join(ROOT, 'gpurun_out', 'bench_detail.json')
        try:
            os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
            with open(path, 'w') as f:
                json.dump({'headline': {k: res[k] for k in LINE_KEYS if k in res}, **detail}, f, indent=1)
        except OSError as e:
            print(f'[bench] could not write {path}: {e}', file=sys.stderr)
        for k in detail.get('kernels', []):
            print(f"[bench] {k['us']:9.2f} us  {k['bound']:4s} frac {k['frac']:.3f}  {k['kernel'][:100]}", file=sys.stderr)
        om = detail.get('other_models')
        for k in (om if isinstance(om, list) else []):
            if 'us' in k:
                print(f"[bench] {k['us']:9.2f} us  {k.get('bound', ''):4s} frac {k.get('frac', 0):.3f}  {k.get('model', '')}: "
                      f"{k.get('kernel', '')[:90]}", file=sys.stderr)
            elif 'ms_per_step' in k:
                print(f"[bench] {k['ms_per_step']:9.2f} ms/step {k.get('images_per_sec')} img/s  {k.get('model')}: "
                      f"{k.get('train_step')}", file=sys.stderr)
        if isinstance(om, dict):
            print(f'[bench] other_models: {om}', file=sys.stderr)
        gr = detail.get('graph_rows')
        for k in (gr if isinstance(gr, list) else []):
            if 'us_eager' in k:
                print(f"[bench] hipGraph {k['head'][:60]:60s} eager {k['us_eager']:8.1f} us  replay {k['us_graph_replay']:8.1f} us  "
                      f"bit-identical {k['bit_identical_to_eager']}", file=sys.stderr)
            else:
                print(f'[bench] hipGraph {k}', file=sys.stderr)
        sys.stderr.flush()
    if seal:         # the real run: nothing may follow the line on this process's stdout (seal_stdout)
        seal_stdout(final_line(res))
    else:
        sys.stdout.flush()
        print(final_line(res), flush=True)


def flush_c_stdio():
    """Native libraries in this process write to the C stdio buffers of stdout (RCCL's version banner sits there until exit):
    push them out NOW, so that nothing of theirs can land behind the line the driver parses."""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass


def seal_stdout(line=None):
    """Print `line` (rank 0: the final JSON line; other ranks: nothing) as the LAST thing this process ever writes to stdout:
    flush python's and C's buffers first, then point fd 1 at /dev/null - a banner flushed at exit, an atexit message of a
    library or a late warning cannot follow the line any more."""
    sys.stdout.flush()
    flush_c_stdio()
    if line is not None:
        os.write(1, (line + '\n').encode())
    try:
        null = os.open(os.devnull, os.O_WRONLY)
        os.dup2(null, 1)
        os.close(null)
    except OSError:
        pass


def main():
    a = parse()
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        respawn_one_rank_per_gpu(a)                        # does not return
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world != a.gpus:
        sys.exit(f'bench.py: --gpus {a.gpus} but WORLD_SIZE={world}')
    from hawkeye_amd import ddp
    if a.share_gpu:
        os.environ['LOCAL_RANK'] = '0'
    use_pg = world > 1 or a.force_pg
    rank, world, local = ddp.init_from_env((a.backend or 'nccl') if use_pg else None, force=a.force_pg)
    assert torch.cuda.is_available(), 'bench.py needs an MI355X'
    dev = torch.device('cuda', local)
    torch.cuda.set_device(dev)
    rank_devices = None
    if world > 1:
        torch.set_num_threads(min(torch.get_num_threads(), host_threads_per_rank(world)))
        # the communicator the gradients will cross must span exactly the ranks the metric counts
        assert torch.distributed.is_initialized() and torch.distributed.get_world_size() == a.gpus == world, \
            (torch.distributed.get_world_size(), a.gpus, world)
        rank_devices = gather_rank_devices(rank, world, dev)
        if not a.share_gpu:
            assert rank_devices['distinct_devices'] == world, f'{world} ranks on {rank_devices}'
    torch.backends.cudnn.benchmark = bool(a.miopen_find)   # MIOpen find mode: pick the fastest conv algorithm once
    torch.manual_seed(0)

    model = build_model(a.model, a.classes).to(dev)
    if a.channels_last:
        model = model.to(memory_format=torch.channels_last)
    model.train()
    crit = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    params = list(model.parameters())
    if a.model in ('OSMENet', 'CIN'):                      # criteria of their own; 7x7 feature maps: 224x224 images
        assert a.image == 224, f'{a.model} heads are built for 7x7 maps: run with --image 224'
        from hawkeye_amd.config import CfgNode
        from hawkeye_amd.model.loss import CINLoss, MAMCLoss
        crit = (MAMCLoss(CfgNode(dict(lambda_a=0.5, use_mamc=True))) if a.model == 'OSMENet'
                else CINLoss(CfgNode(dict(alpha=2.0, beta=0.5))).to(dev))
        params += list(crit.parameters())
    opt = torch.optim.SGD(params, lr=0.005, momentum=0.9, weight_decay=1e-5)   # configs/BCNN_S2
    # (with --full the bucket timeline is always recorded with more than one rank: where in the backward each all-reduce
    #  was issued, without a code change)
    reducer = ddp.GradientAllReducer(model, trace=a.force_pg or a.ddp_trace or (a.full and world > 1)) if use_pg else None

    g = torch.Generator(device=dev).manual_seed(rank)
    images = torch.randn(a.batch, 3, a.image, a.image, device=dev, generator=g)
    if a.channels_last:
        images = images.contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, a.classes, (a.batch,), device=dev, generator=g)
    if a.model in ('OSMENet', 'CIN'):                      # class-balanced batches (pairs of samples per class)
        labels = (torch.arange(a.batch, device=dev) // 2) % a.classes

    def step(keep=False):
        out = model(images, labels) if a.model == 'APCNN' else model(images)
        loss = sum(crit(o, labels) for o in out[1]) if a.model == 'APCNN' else crit(out, labels)   # tuples: MAMC / CIN
        if reducer is not None:
            reducer.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
        loss.backward()
        if reducer is not None:
            reducer.finish()
        opt.step()
        return loss, (out if keep else None)       # keep: the outputs of the step --dump-outputs writes

    kernels_before = None
    if a.full and a.kernels_first and world == 1:
        kernels_before = kernel_rooflines(a.batch, 512, (a.image // 32) ** 2, dev)
    for i in range(a.warmup):
        tw = time.perf_counter()
        step()
        if a.verbose:
            torch.cuda.synchronize()
            print(f'[bench] warmup step {i}: {time.perf_counter() - tw:.2f}s', file=sys.stderr, flush=True)
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss, out = step(keep=a.dump_outputs is not None and i == a.steps - 1)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt.item())
    assert torch.isfinite(loss).item(), 'loss is not finite'

    if rank == 0:
        res = {
            'metric': f'images/sec (train fwd+bwd) {a.model} VGG-16 {a.image}^2 bs{a.batch}' if a.model in ('BCNN', 'CBCNN')
                      else f'images/sec (train fwd+bwd) {a.model} {a.image}^2 bs{a.batch}',
            'value': round(a.batch * world * a.steps / dt, 2), 'unit': 'images/sec',
            'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': round(dt / a.steps * 1e3, 3),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': f'{a.model}_S2: VGG-16 {a.image}x{a.image}, per-GPU batch {a.batch}, {a.classes} classes, '
                                   f'SGD momentum 0.9, CE label_smoothing 0.1, full train step'
                                   if a.model in ('BCNN', 'CBCNN') else f'{a.model} {a.image}x{a.image} batch {a.batch}',
                       'global_batch': a.batch * world, 'parallelism': f'dp{world}',
                       'memory_format': 'channels_last' if a.channels_last else 'contiguous'},
        }
        detail = {}
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, loss, out, model)
        if a.full and world == 1 and not a.no_kernels:
            ks = kernel_rooflines(a.batch, 512, (a.image // 32) ** 2, dev)
            # the step's longest single hand-written launch sequence (stage entry points and multi-launch sums excluded)
            dom = max((k for k in ks if k['shipped_kernel']), key=lambda k: k['us'])
            # (the committed counters were taken at the metric's shape: another shape gets no traffic figure)
            at_profiled_shape = (a.batch, a.image, a.classes) == (64, 448, 200)
            tr_bytes, tr_src = pmc_traffic(dom['kernel']) if at_profiled_shape else (None, None)
            res['roofline'] = {'bound': dom['bound'], 'achieved': dom['achieved'], 'peak': dom['peak'], 'unit': dom['unit'],
                               'frac': dom['frac'], 'traffic': tr_bytes, 'kernel': dom['kernel'][:96], 'us': dom['us'],
                               'flops_algorithmic': dom['flops_algorithmic'], 'flops_executed': dom['flops_executed'],
                               'bytes_algorithmic': dom['bytes_algorithmic'], 'traffic_source': tr_src}
            # the path's own entry points beside the 8(f) classifier kernel above: kernel, us, frac
            res['roofline']['also'] = [{'kernel': k['kernel'].split(',')[0].split(':')[0][:48], 'us': k['us'], 'frac': k['frac'],
                                        'bound': k['bound']}
                                       for k in ks if k['kernel'].startswith(('hk_bcnn_pool_fwd', 'hk_bcnn_pool_bwd_tdot',
                                                                              'hk_linear_fwd'))]
            detail['kernels'] = ks
            if kernels_before is not None:
                detail['kernels_before'] = kernels_before
        if a.full and world == 1 and not a.no_cpu_baseline:
            res['cpu_baseline'] = cpu_baseline(a.image, a.classes)
        if reducer is not None and reducer.trace:
            tl = reducer.timeline()
            detail['ddp_timeline'] = tl
            detail['ddp_buckets_mib'] = [mb for _, mb in reducer.describe()]
            if tl:       # on the line itself: when each gradient bucket's all-reduce was issued inside the backward (ms since zero_grad)
                res['ddp'] = {'buckets_mib': detail['ddp_buckets_mib'], 'issued_ms': [b[2] for b in tl['buckets']],
                              'backward_end_ms': tl['backward_end_ms'], 'joined_ms': tl['joined_ms']}
        if rank_devices is not None:     # who actually ran: ranks, distinct GPUs, backend, host threads per rank
            res.setdefault('ddp', {}).update(
                ranks_seen=rank_devices['ranks_seen'], distinct_devices=rank_devices['distinct_devices'],
                devices=rank_devices['devices'][:8], backend=torch.distributed.get_backend(),
                comm_size=torch.distributed.get_world_size(), host_threads_per_rank=torch.get_num_threads())
        if use_pg:                       # what RCCL built for this communicator (ddp._arm_rccl_log): channels, transports, algorithm
            rs = ddp.rccl_summary(max_lines=2)
            if rs is not None:
                detail['rccl'] = ddp.rccl_summary(max_lines=40)
                res.setdefault('ddp', {})['rccl'] = {k: rs[k] for k in ('version', 'channels', 'rings', 'trees', 'transports')} | \
                    {'tuning': [t[:80] for t in rs['tuning']]}
        if a.full and world == 1 and not a.no_other_models and a.model == 'BCNN' and not a.force_pg:
            torch.cuda.empty_cache()
            detail['other_models'] = other_models()
            detail['graph_rows'] = graph_rows()
        if world > 1:               # every other rank has sealed its stdout before rank 0 writes the line (below)
            torch.distributed.barrier()
        emit(res, detail, seal=True)
    elif world > 1:
        seal_stdout()
        torch.distributed.barrier()
    if use_pg:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
