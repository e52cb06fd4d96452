#!/usr/bin/env python3
"""bench.py — pair-decode throughput of the MI355X decoding engine on synthetic read pairs.

One "step" = one pass of the hot path (pair_decode_helper's stage chain: two 1-D Viterbi
basecalls, banded alignment, envelope, pair beam search — all on the GPU, through the C-ABI of
include/poreover_hip.h) over this rank's shard of synthetic pairs, with the log-probability
matrices ALREADY RESIDENT IN HBM when the timed region starts.

Workload (the configuration BASELINE.json's metric is quoted on): ONE job of 10 000 synthetic pairs, T ~ 4000
frames, C = 5, CLI defaults (beam width 5, method row_col, banded alignment, padding 5).
N = 1: the rank decodes the 10 000 pairs.  N > 1 (round 6): the headline `value` is the SAME job split over the N ranks
(BASELINE config 4: "10k-pair batched pair-decode sharded across 8 GPUs"; rank r holds pairs [r P / N, (r + 1) P / N) resident
in its HBM, no data-path collective, results stay on the rank) — `"scaling": "strong"`.  A 1 250-pair shard leaves most of a
device's 4 096 pair slots empty and a pair is one serial chain of ~ 14 ms, so this figure scales far below N; the WEAK figure
(every rank its own 10 000 pairs: N x the work) is measured in the same run and reported beside it as `weak_scaling`.
`strong_scaling` is the same one job END TO END: host float32 logit matrices in -> Python strings out (H2D, device
log-softmax, decode, D2H, string building all on the clock), split over the N ranks; at N = 1 that is the end-to-end figure
(`e2e`).  `--inprocess_devices 0,1,...` measures that job driven by ONE process over several devices (po_multi_pair_decode),
the product's path on a multi-GPU node outside torchrun.  `--share_device` puts every rank on device 0 (the tests' way to run
the N > 1 code on a one-GPU box; the figures mean nothing then).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--pairs P] [--T 4000] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run generates the inputs, warms up, times the K steps and prints the headline (`value`, `ms_per_step`,
`mbases_per_s`, `config`).  Everything else this script measures or checks runs only with `--full`: the CPU baseline,
the per-kernel timers and both rooflines, the parity check against the oracle's digests, the weak-scaling and
end-to-end legs, the two-stream rate and the secondary configurations (`--no_strong`, `--no_secondary`, `--no_weak`,
`--cpu_sample` and `--inprocess_devices` select among them).  `--dump-outputs DIR` writes what the last timed step
returned (rank 0's pairs) as .npy files; the inputs are seeded, so two builds can be compared output for output.

`--gpus N` (N > 1) outside a torchrun environment starts the N ranks itself (a fresh torch.distributed.run child,
created before this process has touched torch or HIP) and relays rank 0's line; the reported n_gpus is always the
number of ranks that ran.

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for the byte accounting).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
# the pair beam search kernel this workload runs on (row_col, ctc, W = 5): name prefix in the profiles
# (profiles before the row_col-only instantiation existed call it beam2d_kernel<0, 6>, later ones beam2d_kernel<0, 6, true>;
#  PO_RING_AUTO=1 makes the LDS-ring kernel the engine's choice: an A/B switch)
#  since round 4 the register-state kernel beam2d_reg_kernel is the engine's choice at every batch size; PO_REG_NEVER=1
#  sends the launch to beam2d_kernel for the A/B)
LEGACY = bool(os.environ.get("PO_REG_NEVER"))
MAIN_KERNEL = "beam2d_kernel<0, 6" if LEGACY else "beam2d_reg_kernel"


def _cpu_pair_worker(args):
    """Decode a few pairs on one host core: C port for the glue stages + the reference's own C++
    (oracle/_ref) for the pair beam search when it is available."""
    seeds, T, use_ref = args
    from oracle import po_oracle as O
    from poreover_amd.synth import synth_pair
    t_total, bases = 0.0, 0
    for sd in seeds:
        y1, y2 = synth_pair(sd, T=T)
        t0 = time.perf_counter()
        s1, p1 = O.viterbi_decode(y1)                                   # pair_decode.py:360-362
        s2, p2 = O.viterbi_decode(y2)
        m1, m2 = O.get_sequence_mapping(p1, "poreover"), O.get_sequence_mapping(p2, "poreover")
        a1, a2 = O.global_pair_banded(s1, s2)                            # :389
        ident = sum(x == y for x, y in zip(a1, a2)) / len(a1)
        if abs(len(s1) - len(s2)) <= 1000 and ident >= 0.5:
            env = O.build_envelope(len(y1), len(y2), a1, a2, m1, m2, 5)  # :500-501
            beam = O.ref_beam_search_2d if use_ref else O.cpp_beam_search_2d
            bases += len(beam(y1, y2, env, 5, method_="row_col"))        # :511
        t_total += time.perf_counter() - t0
    return t_total, bases, len(seeds)


def cpu_baseline(T, sample_pairs):
    """Bounded CPU sample of the same workload on this host's cores (mirrors --threads N)."""
    import multiprocessing as mp
    from oracle import po_oracle as O
    O.build()
    use_ref = O.have_ref()
    cores = max(1, min(os.cpu_count() or 1, 32))
    per = max(1, sample_pairs // cores)
    jobs = [([900000 + c * per + i for i in range(per)], T, use_ref) for c in range(cores)]
    t0 = time.perf_counter()
    with mp.get_context("fork").Pool(cores) as pool:
        res = pool.map(_cpu_pair_worker, jobs)
    wall = time.perf_counter() - t0
    n = sum(r[2] for r in res)
    busy = sum(r[0] for r in res)
    return {
        "value": round(n / (busy / cores), 3),     # aggregate pairs/s with all `cores` busy
        "unit": "read-pairs/s",
        "cores": cores,
        "kind": "reference" if use_ref else "port",
        "wall_value": round(n / wall, 3),       # the same sample by the wall clock (pool start-up and stragglers included)
        "per_core": round(n / busy, 3),
        "mbases_per_s": round(sum(r[1] for r in res) / (busy / cores) / 1e6, 6),
        "sample": ("%d synthetic pairs (T~%d, W=5 row_col) on %d processes, %.1f s wall; pair beam search = "
                   "%s, glue stages (Viterbi, banded NW, envelope) = C port of the reference's Python/Cython"
                   % (n, T, cores, wall,
                      "the reference's own C++ (oracle/_ref)" if use_ref else "C port (oracle/_ref not built)")),
    }


def _self_launch(gpus):
    """--gpus N without RANK / WORLD_SIZE in the environment: become the launcher.  Nothing in this process has
    imported torch or initialised HIP; the ranks are children of a fresh torch.distributed.run process."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    raise SystemExit(subprocess.call(cmd, env=env))


def _digest(seq1, seq2, cons):
    import hashlib
    return hashlib.md5(("%s|%s|%s" % (seq1, seq2, cons)).encode()).hexdigest()[:10]


DUMP_BYTES = 64 << 20   # --dump-outputs writes at most this much
DUMP_SAMPLE = 1000      # at most this many pairs have their strings and envelope written


def dump_outputs(path, o1, s1o, so, d_seq1d, d_l1, d_l2, d_id, d_env, d_seq, d_len, d_st):
    """--dump-outputs: what po_pair_decode_batch returned, masked as batch.pair_decode_batch hands it to its callers.
    Every pair: status, length1, length2, consensus_length (0 unless decoded) and sequence_identity (NaN after a length
    skip), float64.  A seeded sample of pairs (`sample_pairs`, ascending; chosen from the input shapes alone, as many as
    fit in DUMP_BYTES): seq1, seq2 and consensus as float32 character codes and envelope as float32 (rows, 2), each
    concatenated over the sampled pairs in that order."""
    import torch
    from poreover_amd import _lib
    os.makedirs(path, exist_ok=True)
    st = d_st.cpu().numpy()
    n = len(st)
    ok = st == 0
    called = ok | (st == _lib.SKIP_LENGTH) | (st == _lib.SKIP_IDENTITY)
    l1 = np.where(called, d_l1.cpu().numpy(), 0)
    l2 = np.where(called, d_l2.cpu().numpy(), 0)
    lens = np.where(ok, d_len.cpu().numpy(), 0)
    ident = np.where(called & (st != _lib.SKIP_LENGTH), d_id.cpu().numpy(), np.nan)
    # bytes a sampled pair can take at most: both basecalls and the consensus at their capacity, two bounds per row
    rows1 = np.diff(o1)
    cost = 4 * ((s1o[2::2] - s1o[0:-1:2]) + np.diff(so) + 2 * rows1)
    budget = DUMP_BYTES - 6 * 8 * n - (1 << 20)   # (the per-pair arrays, sample_pairs and the .npy headers first)
    order = np.random.default_rng(20240).permutation(n)[:DUMP_SAMPLE]
    take = np.sort(order[:int(np.searchsorted(np.cumsum(cost[order]), budget, side="right"))])

    def gather(d, spans):
        spans = [(int(a), int(b)) for a, b in spans if b > a]
        return torch.cat([d[a:b] for a, b in spans]).cpu().numpy().astype(np.float32) if spans else np.zeros(0, np.float32)
    arrays = {
        "status": st.astype(np.float64), "length1": l1.astype(np.float64), "length2": l2.astype(np.float64),
        "consensus_length": lens.astype(np.float64), "sequence_identity": ident.astype(np.float64),
        "sample_pairs": take.astype(np.float64),
        "seq1": gather(d_seq1d, [(s1o[2 * i], s1o[2 * i] + l1[i]) for i in take]),
        "seq2": gather(d_seq1d, [(s1o[2 * i + 1], s1o[2 * i + 1] + l2[i]) for i in take]),
        "consensus": gather(d_seq, [(so[i], so[i] + lens[i]) for i in take]),
        "envelope": gather(d_env, [(2 * o1[i], 2 * o1[i + 1]) for i in take if ok[i]]).reshape(-1, 2),
    }
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=10000, help="pairs per GPU")
    ap.add_argument("--T", type=int, default=4000)
    ap.add_argument("--beam_width", type=int, default=5)
    ap.add_argument("--gen_procs", type=int, default=0, help="processes generating the synthetic inputs (0 = auto; use 1 under "
                    "rocprofv3, whose preloaded library initialises the GPU before Python starts, which makes fork unsafe)")
    ap.add_argument("--cpu_sample", type=int, default=512, help="pairs decoded on the CPU for the baseline (0 = skip)")
    ap.add_argument("--e2e_wave_pairs", type=int, default=0, help="pairs per wave of the end-to-end pipeline leg (0 = the library's default)")
    ap.add_argument("--no_strong", action="store_true", help="skip the strong-scaling / end-to-end leg (host arrays -> strings)")
    ap.add_argument("--inprocess_devices", type=str, default="", help="comma-separated device list: also time the 10k-pair job "
                    "driven by ONE process over these devices (po_multi_pair_decode); single-process runs only")
    ap.add_argument("--no_secondary", action="store_true", help="skip the secondary configurations (1-D beam, flip-flop, "
                    "single-pair latency, end-to-end) measured after the timed region at N = 1")
    ap.add_argument("--share_device", action="store_true", help="every rank on device 0 (testing the N > 1 path on a one-GPU box)")
    ap.add_argument("--no_weak", action="store_true", help="N > 1: skip the weak-scaling leg (every rank its own P pairs)")
    ap.add_argument("--full", action="store_true", help="also run every measurement and check beside the headline (CPU "
                    "baseline, per-kernel timers and rooflines, digest parity, weak / end-to-end / two-stream / secondary legs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the outputs of the last timed step (rank 0) "
                    "as DIR/<name>.npy")
    args = ap.parse_args()

    if "RANK" not in os.environ and "WORLD_SIZE" not in os.environ and args.gpus > 1:
        _self_launch(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.share_device else int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    args.gpus = world   # n_gpus in the report = the ranks that actually run

    # ---- everything that forks worker processes happens BEFORE the GPU runtime is initialised
    # (forking a process that holds a HIP context is unsafe, in particular under rocprofv3)
    from poreover_amd import dist as podist
    from poreover_amd.batch import pack_rows
    from poreover_amd.synth import synth_pair
    P, T = args.pairs, args.T
    nproc = args.gen_procs if args.gen_procs > 0 else max(1, min(16, (os.cpu_count() or 1) // max(1, world)))

    def gen(seed_list):
        if nproc > 1 and len(seed_list) >= 256:
            import multiprocessing as mp
            with mp.get_context("fork").Pool(nproc) as pool:
                return pool.starmap(synth_pair, [(sd, T) for sd in seed_list], chunksize=32)
        return [synth_pair(sd, T=T) for sd in seed_list]
    # the ONE job: seeds 0 .. P - 1; this rank's share [slo, shi) (N = 1: all of it)
    slo, shi = podist.shard_range(P, rank, world)
    job_pairs = gen(list(range(slo, shi)))
    y1, o1, Cc = pack_rows([p[0] for p in job_pairs])
    y2, o2, _ = pack_rows([p[1] for p in job_pairs])
    strong_pairs = job_pairs if (args.full and world > 1 and not args.no_strong) else None   # (N = 1: the end-to-end leg slices y1 / y2)
    del job_pairs
    # weak scaling (N > 1 only): every rank its OWN P pairs, the seeds of rounds 1 - 5 (rank 0: the job's)
    weak_in = None
    if args.full and world > 1 and not args.no_weak:
        wp_ = gen(list(podist.shard_seeds(P, rank)))
        weak_in = (pack_rows([p[0] for p in wp_]), pack_rows([p[1] for p in wp_]))
        del wp_
    secondary = args.full and rank == 0 and world == 1 and not args.no_secondary
    ff_reads = None
    if secondary:   # BASELINE config 5: 1 000 flip-flop reads (T x 8)
        from poreover_amd.synth import synth_read
        nff = min(1000, P)
        if nproc > 1:
            import multiprocessing as mp
            with mp.get_context("fork").Pool(nproc) as pool:
                ff_reads = pool.starmap(synth_read, [(500000 + i, T, 0, True) for i in range(nff)], chunksize=16)
        else:
            ff_reads = [synth_read(500000 + i, T, 0, True) for i in range(nff)]
    ff_pairs = None
    if secondary:   # flip-flop PAIRS for the secondary pair-decode line (T x 8 tables, 5 GB of float64 for 10 000 pairs)
        nfp = P
        if nproc > 1:
            import multiprocessing as mp
            with mp.get_context("fork").Pool(nproc) as pool:
                ff_pairs = pool.starmap(synth_pair, [(700000 + i, T, 0, True) for i in range(nfp)], chunksize=16)
        else:
            ff_pairs = [synth_pair(700000 + i, T=T, flipflop=True) for i in range(nfp)]
    cpu_base = None
    if args.full and rank == 0 and args.gpus == 1 and world == 1 and args.cpu_sample > 0:
        cpu_base = cpu_baseline(T, args.cpu_sample)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X GPU (no CPU fallback exists)")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # (the timing barrier and the max / sum of a few floats: gloo does that without touching the fabric — north_star: RCCL
        #  unused; rounds 1 - 4 initialised an nccl group for it)
        dist.init_process_group("gloo")

    from poreover_amd import _lib
    lib = _lib.load()
    _lib.set_device(local_rank)   # (binds the library AND tells the cached pipelines of the strong-scaling leg which device they are on)

    Pl = shi - slo   # pairs of the job on this rank (N = 1: P)
    tr1, tr2 = int(o1[-1]), int(o2[-1])
    mr1, mr2 = int(np.diff(o1).max()), int(np.diff(o2).max())
    s1o = np.zeros(2 * Pl + 1, dtype=np.int64)
    caps = np.empty(2 * Pl, dtype=np.int64)
    caps[0::2], caps[1::2] = np.diff(o1), np.diff(o2)
    np.cumsum(caps, out=s1o[1:])
    so = np.zeros(Pl + 1, dtype=np.int64)
    np.cumsum(np.diff(o1) + np.diff(o2), out=so[1:])

    dev = torch.device("cuda", local_rank)
    d_y1 = torch.from_numpy(y1).to(dev)
    d_y2 = torch.from_numpy(y2).to(dev)
    d_o1, d_o2 = torch.from_numpy(o1).to(dev), torch.from_numpy(o2).to(dev)
    d_s1o, d_so = torch.from_numpy(s1o).to(dev), torch.from_numpy(so).to(dev)
    d_seq1d = torch.empty(int(s1o[-1]), dtype=torch.uint8, device=dev)
    d_seq = torch.empty(int(so[-1]), dtype=torch.uint8, device=dev)
    d_l1, d_l2, d_len, d_st = (torch.zeros(Pl, dtype=torch.int32, device=dev) for _ in range(4))
    d_id = torch.zeros(Pl, dtype=torch.float64, device=dev)
    d_env = torch.zeros(2 * tr1, dtype=torch.int32, device=dev)
    opt = _lib.PairOptions(args.beam_width, _lib.MODELS["ctc"], _lib.METHODS["row_col"], 5, 0, 0, 50)
    wsb = lib.po_pair_decode_workspace_bytes(Pl, tr1, tr2, mr1, mr2, Cc, C.byref(opt))
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    # The timed region issues its steps one after the other on ONE stream (the contract's step; what rounds 1 - 3 report as
    # `value`).  `two_streams` (after the timed region, reported beside it): the same steps issued to two streams in turn,
    # each with its own outputs and workspace (the inputs are read-only), the way the pipelined host layer issues its waves —
    # the tail of one step's launches, the last pair of every workgroup on a device that is emptying, is filled by the next
    # step's first pairs.
    sets = [(d_seq1d, d_l1, d_l2, d_id, d_env, d_seq, d_len, d_st, d_ws, stream)]
    step_no = [0]

    def step():
        q1d, ql1, ql2, qid, qenv, qseq, qlen, qst, qws, qstream = sets[step_no[0] % len(sets)]
        step_no[0] += 1
        _lib.check(lib.po_pair_decode_batch(
            d_y1.data_ptr(), d_o1.data_ptr(), d_y2.data_ptr(), d_o2.data_ptr(), Pl, Cc, C.byref(opt),
            q1d.data_ptr(), d_s1o.data_ptr(), ql1.data_ptr(), ql2.data_ptr(), qid.data_ptr(),
            qenv.data_ptr(), qseq.data_ptr(), d_so.data_ptr(), qlen.data_ptr(), qst.data_ptr(),
            qws.data_ptr(), wsb, qstream), "po_pair_decode_batch")

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    if args.full:   # per-kernel HIP events around the launches: the rooflines' kernel times
        lib.po_profile_enable(1)
        lib.po_profile_reset()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:   # (before anything below launches into the same output buffers)
        dump_outputs(args.dump_outputs, o1, s1o, so, d_seq1d, d_l1, d_l2, d_id, d_env, d_seq, d_len, d_st)
    if args.full:
        lib.po_profile_enable(0)
        # update_prob evaluations (reference schedule, executed) of ONE more step, outside the timed region: with the counter
        # attached the kernels count per step (ballots, a wave reduction per scan) — diagnostics the product path does not run
        d_upd = torch.zeros(2, dtype=torch.int64, device=dev)
        lib.po_profile_update_counter(d_upd.data_ptr())
        step()
        barrier()
        lib.po_profile_update_counter(None)
        n_upd, n_upd_exec = (int(x) * args.steps for x in d_upd.cpu().tolist())   # (every step decodes the same pairs)

    # ---- N > 1: the WEAK figure beside the headline — every rank its own P pairs resident, the same W + K steps and clock
    weak = None
    if weak_in is not None:
        (wy1, wo1, _), (wy2, wo2, _) = weak_in
        wt1, wt2 = int(wo1[-1]), int(wo2[-1])
        ws1 = np.zeros(2 * P + 1, dtype=np.int64)
        wc = np.empty(2 * P, dtype=np.int64)
        wc[0::2], wc[1::2] = np.diff(wo1), np.diff(wo2)
        np.cumsum(wc, out=ws1[1:])
        wso = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(np.diff(wo1) + np.diff(wo2), out=wso[1:])
        w_y1, w_y2 = torch.from_numpy(wy1).to(dev), torch.from_numpy(wy2).to(dev)
        w_o1, w_o2 = torch.from_numpy(wo1).to(dev), torch.from_numpy(wo2).to(dev)
        w_s1o, w_so = torch.from_numpy(ws1).to(dev), torch.from_numpy(wso).to(dev)
        w_seq1d = torch.empty(int(ws1[-1]), dtype=torch.uint8, device=dev)
        w_seq = torch.empty(int(wso[-1]), dtype=torch.uint8, device=dev)
        w_l1, w_l2, w_len, w_st = (torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(4))
        w_id = torch.zeros(P, dtype=torch.float64, device=dev)
        w_env = torch.zeros(2 * wt1, dtype=torch.int32, device=dev)
        wwsb = lib.po_pair_decode_workspace_bytes(P, wt1, wt2, int(np.diff(wo1).max()), int(np.diff(wo2).max()), Cc, C.byref(opt))
        w_ws = torch.empty(wwsb, dtype=torch.uint8, device=dev)

        def wstep():
            _lib.check(lib.po_pair_decode_batch(
                w_y1.data_ptr(), w_o1.data_ptr(), w_y2.data_ptr(), w_o2.data_ptr(), P, Cc, C.byref(opt),
                w_seq1d.data_ptr(), w_s1o.data_ptr(), w_l1.data_ptr(), w_l2.data_ptr(), w_id.data_ptr(),
                w_env.data_ptr(), w_seq.data_ptr(), w_so.data_ptr(), w_len.data_ptr(), w_st.data_ptr(),
                w_ws.data_ptr(), wwsb, stream), "po_pair_decode_batch")
        for _ in range(args.warmup):
            wstep()
        barrier()
        tw = time.perf_counter()
        for _ in range(args.steps):
            wstep()
        barrier()
        w_elapsed = time.perf_counter() - tw
        wst_, wln_ = w_st.cpu().numpy(), w_len.cpu().numpy()
        w_bases = int(wln_[wst_ == 0].sum())
        wmax, (w_pairs, w_tb) = podist.job_aggregate(dist, w_elapsed, [P * args.steps, w_bases * args.steps], dev)
        weak = {"value": round(w_pairs / wmax, 3), "unit": "read-pairs/s", "mbases_per_s": round(w_tb / wmax / 1e6, 4),
                "ms_per_step": round(wmax / args.steps * 1e3, 3), "pairs_per_gpu": P, "scaling": "weak",
                "note": "every rank its own %d pairs (N x the work of the headline's one job): what rounds 1 - 5 reported as `value`" % P}
        del w_y1, w_y2, w_seq1d, w_seq, w_ws, w_env, weak_in
        torch.cuda.empty_cache()

    def _kernel_ms(k):
        ms, cnt = C.c_double(), C.c_int64()
        lib.po_profile_get(k, C.byref(ms), C.byref(cnt))
        return ms.value, cnt.value
    # (read now: the secondary configurations below use the same per-kernel timers)
    prof = {k: _kernel_ms(k) for k in (_lib.K_BEAM2D, _lib.K_VITERBI, _lib.K_ALIGN, _lib.K_BEAM2D_MAIN)} if args.full else None
    lae_peak = C.c_double(0.0)
    if args.full and rank == 0:   # outside the timed region: the device's peak rate of the engine's logaddexp
        _lib.check(lib.po_lae_peak(20000, C.byref(lae_peak), stream), "po_lae_peak")

    st = d_st.cpu().numpy()
    lens = d_len.cpu().numpy()
    decoded = int((st == 0).sum())
    bases = int(lens[st == 0].sum())
    bad = int(((st != 0) & (st != _lib.SKIP_LENGTH) & (st != _lib.SKIP_IDENTITY)).sum())
    if bad:
        raise SystemExit("bench.py: %d pairs failed with an engine error (first code %d)" % (bad, int(st[(st != 0)][0])))

    # ---- parity of what was just timed: the first pairs of rank 0 against the committed digests of the oracle's
    # results for the same seeds (tests/golden/batch_digest.json) — strings, not only statuses
    parity = None
    if args.full and rank == 0 and T == 4000 and args.beam_width == 5:
        try:
            with open(os.path.join(REPO, "tests", "golden", "batch_digest.json")) as f:
                dig = json.load(f)["records"]
            k = min(Pl, len(dig))
            h_seq = d_seq[: int(so[k])].cpu().numpy().tobytes()
            h_s1 = d_seq1d[: int(s1o[2 * k])].cpu().numpy().tobytes()
            h_l1, h_l2 = d_l1[:k].cpu().numpy(), d_l2[:k].cpu().numpy()
            bad_dig = 0
            for i in range(k):
                a = h_s1[s1o[2 * i]: s1o[2 * i] + h_l1[i]].decode()
                b = h_s1[s1o[2 * i + 1]: s1o[2 * i + 1] + h_l2[i]].decode()
                c = h_seq[so[i]: so[i] + lens[i]].decode() if st[i] == 0 else ""
                if [int(st[i]), len(a), len(b), len(c), _digest(a, b, c)] != dig[i]:
                    bad_dig += 1
            parity = {"pairs_checked": k, "digest_mismatches": bad_dig, "chain_mode": _lib.get_chain_mode(),
                      "against": "tests/golden/batch_digest.json (CPU oracle, same seeds)"}
            # The engine's default arithmetic is the reference's chain by chain: ANY differing string fails the run (round 5
            # allowed one pair in a thousand here and in the secondary legs; a rare kernel regression — round 5's own was 1 pair
            # in 83 000 — would have passed).  north_star's budget (<= 0.1 % edits where float ties reorder; in digests: one pair
            # in a thousand) is what the opt-in closed-form chain mode is held to.
            if bad_dig > (k // 1000 if _lib.get_chain_mode() != "serial" else 0):
                raise SystemExit("bench.py: %d of %d decoded pairs differ from the oracle's digests" % (bad_dig, k))
        except FileNotFoundError:
            parity = None

    # ---- strong scaling / end to end: ONE job of P pairs, host float32 logit matrices (the form the .npy files hold)
    # in -> Python strings out through the pipelined host layer (pack -> H2D -> device ingest -> decode -> D2H, two
    # slots), this rank's share [slo, shi) on its own device; the clock is the slowest rank's
    # (This leg runs BEFORE the secondary configurations since round 4: after them — ~ 20 s of other kernels, their host
    #  lists and device buffers — the same job measured 69 - 71k pairs/s where it reaches 85 - 93k on a fresh process
    #  (gpurun_out/r04_g38: packing 31 instead of 20 ms, H2D 11 instead of 14 GB/s); what is measured is the pipeline, not the
    #  state the other legs leave the host in.)
    strong = None
    if args.full and not args.no_strong:
        from poreover_amd import batch as pobatch
        torch.cuda.empty_cache()
        if os.environ.get("PO_BENCH_SETTLE"):   # experiment: let the driver finish with the memory just freed
            torch.cuda.synchronize(); time.sleep(float(os.environ["PO_BENCH_SETTLE"]))
        if strong_pairs is None:
            l1s = [y1[o1[i]:o1[i + 1]].astype(np.float32) for i in range(Pl)]
            l2s = [y2[o2[i]:o2[i + 1]].astype(np.float32) for i in range(Pl)]
        else:
            l1s = [q[0].astype(np.float32) for q in strong_pairs]
            l2s = [q[1].astype(np.float32) for q in strong_pairs]
            strong_pairs = None
        ns = len(l1s)
        wp = args.e2e_wave_pairs
        # The FIRST full-size call of this process through the pipelined host layer is reported by itself (`first_call_s`: the
        # pipeline is created, its pinned staging ring and every device buffer are allocated inside it — what a one-shot
        # `python -m poreover_amd pair-decode` pays on top of HIP's own start-up, which this process has behind it).  No
        # small warm-up call: round 4 warmed up with 256 pairs and hid a 2 s first repetition behind a median.
        barrier()
        t0 = time.perf_counter()
        pobatch.pair_decode_stream(l1s, l2s, "poreover", args.beam_width, "row_col", wave_pairs=wp)
        first_call_s, _ = podist.job_aggregate(dist, time.perf_counter() - t0, [0], dev)
        runs, stt, res = [], {}, None
        for _ in range(3):   # the MEDIAN of three further repetitions is reported, with the spread beside it
            barrier()
            t0 = time.perf_counter()
            res = pobatch.pair_decode_stream(l1s, l2s, "poreover", args.beam_width, "row_col", stats=stt, wave_pairs=wp)
            dt_local = time.perf_counter() - t0
            sb = sum(len(r["consensus"] or "") for r in res)
            dt, (tb,) = podist.job_aggregate(dist, dt_local, [sb], dev)
            runs.append((dt, tb))
        runs.sort()
        best = runs[len(runs) // 2]
        in_bytes = 4.0 * Cc * (tr1 + tr2) * world   # float32 logits of the whole job (every rank holds ~ 1 / N of it)
        strong = {"pairs": P, "n_gpus": world, "seconds": round(best[0], 4), "pairs_per_s": round(P / best[0], 1),
                  "first_call_s": round(first_call_s, 4), "first_call_pairs_per_s": round(P / first_call_s, 1),
                  "repetitions": len(runs), "seconds_min": round(runs[0][0], 4), "seconds_max": round(runs[-1][0], 4),
                  "pairs_per_s_min": round(P / runs[-1][0], 1), "pairs_per_s_max": round(P / runs[0][0], 1),
                  "mbases_per_s": round(best[1] / best[0] / 1e6, 3),
                  "h2d_gbps": round(in_bytes / best[0] / 1e9, 2),
                  "mode": "one process per GPU (this launch), each rank its 1/N share of the same %d host arrays" % P,
                  "input": "list of host float32 logit matrices (T x 5), 80 KB per read over PCIe", "output": "Python strings",
                  "pipeline_rank0": dict(stt)}
        if world == 1 and ns >= 2500:
            # one GPU's share of the 8-GPU strong-scaling job (bench seeds 1250 .. 2499), end to end on this GPU: what the
            # 8-GPU figure can be predicted from (a 1 250-pair launch is latency-bound: a pair is one serial chain on one wave)
            sh = []
            for _ in range(3):
                t0 = time.perf_counter()
                pobatch.pair_decode_stream(l1s[1250:2500], l2s[1250:2500], "poreover", args.beam_width, "row_col")
                sh.append(time.perf_counter() - t0)
            sh.sort()
            strong["shard_1250_e2e"] = {"pairs": 1250, "seconds": round(sh[1], 4), "pairs_per_s": round(1250 / sh[1], 1),
                                        "seconds_min": round(sh[0], 4), "seconds_max": round(sh[2], 4),
                                        "x8_prediction_pairs_per_s": round(10000 / sh[1], 1)}
        if world == 1 and args.inprocess_devices:
            devs = [int(x) for x in args.inprocess_devices.split(",") if x.strip() != ""]
            pobatch.pair_decode_stream(l1s, l2s, "poreover", args.beam_width, "row_col", wave_pairs=wp, devices=devs)
            bi, sti = None, {}
            for _ in range(2):
                t0 = time.perf_counter()
                pobatch.pair_decode_stream(l1s, l2s, "poreover", args.beam_width, "row_col", stats=sti, wave_pairs=wp, devices=devs)
                dt = time.perf_counter() - t0
                bi = dt if bi is None else min(bi, dt)
            strong["inprocess"] = {"devices": devs, "seconds": round(bi, 4), "pairs_per_s": round(P / bi, 1),
                                   "mode": "ONE process, a pipeline and a host thread per device (po_multi_pair_decode)",
                                   "per_device": sti.get("per_device")}
        del l1s, l2s, res

    # (the two-streams leg runs AFTER the end-to-end leg since round 5: measured before it, the end-to-end job of the same process
    #  took 0.123 s instead of 0.096 s — gpurun_out/r05_b9.json vs r05_b7.json — whatever the second set of buffers and streams
    #  leaves behind, the pipeline is what that leg is there to measure)
    two_streams = None
    if rank == 0 and secondary:   # sustained rate with consecutive steps on two streams (see `sets` above)
        s2 = torch.cuda.Stream(device=dev)
        sets.append((torch.empty_like(d_seq1d), torch.zeros_like(d_l1), torch.zeros_like(d_l2), torch.zeros_like(d_id),
                     torch.zeros_like(d_env), torch.empty_like(d_seq), torch.zeros_like(d_len), torch.zeros_like(d_st),
                     torch.empty(wsb, dtype=torch.uint8, device=dev), s2.cuda_stream))
        step_no[0] = 0
        step(); step()
        torch.cuda.synchronize()
        k2 = max(4, args.steps)
        tq = time.perf_counter()
        for _ in range(k2):
            step()
        torch.cuda.synchronize()
        dq = time.perf_counter() - tq
        two_streams = {"value": round(P * k2 / dq, 1), "unit": "read-pairs/s", "steps": k2, "ms_per_step": round(dq / k2 * 1e3, 3),
                       "note": "NOT the headline: the same steps issued to two streams in turn (own outputs and workspace each), as "
                               "the pipelined host layer issues its waves; the next step's first pairs fill the tail of the previous one"}
        del sets[1]
        step_no[0] = 0
    sec = {}
    if secondary:
        # what the oracle returns for these legs' inputs (tests/golden/secondary_digest.json, made by make_secondary_digest.py
        # on the CPU): every leg's strings are compared, not only its statuses
        try:
            with open(os.path.join(REPO, "tests", "golden", "secondary_digest.json")) as f:
                sec_dig = json.load(f)["legs"] if T == 4000 else {}
        except FileNotFoundError:
            sec_dig = {}

        def _md5(*parts):
            import hashlib
            return hashlib.md5("|".join(parts).encode()).hexdigest()[:10]

        def _status_counts(st_arr):
            u, cnt = np.unique(np.asarray(st_arr), return_counts=True)
            return {str(int(a)): int(b) for a, b in zip(u, cnt)}

        def timed(fn, reps=3):
            ev = [(lib.po_event_create(), lib.po_event_create()) for _ in range(reps)]
            fn()
            torch.cuda.synchronize()
            for a_, b_ in ev:
                lib.po_event_record(a_, stream); fn(); lib.po_event_record(b_, stream)
            ms = []
            for a_, b_ in ev:
                f = C.c_float()
                lib.po_event_elapsed_ms(a_, b_, C.byref(f)); ms.append(f.value)
                lib.po_event_destroy(a_); lib.po_event_destroy(b_)
            return sorted(ms)[len(ms) // 2]

        def beam1d_config(d_y, d_off, n, Cn, rows, maxrows, model, W, digest_key=""):
            d_so = d_off
            d_sq = torch.empty(rows, dtype=torch.uint8, device=dev)
            d_ln = torch.zeros(n, dtype=torch.int32, device=dev)
            d_stt = torch.zeros(n, dtype=torch.int32, device=dev)
            wsz = lib.po_beam1d_workspace_bytes(n, rows, maxrows, Cn, W, _lib.MODELS[model])
            d_w = torch.empty(wsz, dtype=torch.uint8, device=dev)
            ms = timed(lambda: _lib.check(lib.po_beam1d_batch(d_y.data_ptr(), d_off.data_ptr(), n, Cn, b"ACGT", W, _lib.MODELS[model],
                                                              d_sq.data_ptr(), d_so.data_ptr(), d_ln.data_ptr(), d_stt.data_ptr(),
                                                              d_w.data_ptr(), wsz, stream), "po_beam1d_batch"))
            h_stt = d_stt.cpu().numpy()
            assert int((h_stt != 0).sum()) == 0
            nb = int(d_ln.sum().item())
            check = None
            if digest_key in sec_dig:   # strings against the oracle's digests for the same reads
                want = sec_dig[digest_key]
                kk = min(n, len(want))
                h_ln, h_o = d_ln[:kk].cpu().numpy(), d_so[:kk + 1].cpu().numpy()
                h_sq = d_sq[: int(h_o[kk])].cpu().numpy().tobytes()
                badd = sum(1 for i in range(kk) if [int(h_stt[i]), int(h_ln[i]), _md5(h_sq[h_o[i]: h_o[i] + h_ln[i]].decode())] != want[i])
                check = {"checked": kk, "mismatches": badd, "statuses": _status_counts(h_stt)}
                if badd:
                    raise SystemExit("bench.py: %s: %d of %d reads differ from the oracle's digests" % (digest_key, badd, kk))
            # what bounds it: T serial steps per read, one wave per read (latency), not HBM and not the VALU — both
            # fractions are reported so that nobody has to take that on trust.  Algorithmic bytes 8*T*C + L per read;
            # update_prob evaluations: every beam node and every child once per frame (W * (A + 1) * logaddexp-per-update).
            lae_per_update = {"ctc": 1, "ctc_merge_repeats": 2, "ctc_flipflop": 3}[model]   # (po_device.h::po_update)
            evals = float(rows) * W * 5 * lae_per_update
            return {"reads": n, "beam_width": W, "kernel_ms": round(ms, 3), "reads_per_s": round(n / ms * 1e3, 1),
                    "mbases_per_s": round(nb / ms / 1e3, 3),
                    "us_per_frame": round(ms * 1e3 / max(maxrows, 1), 3),
                    "roofline": {"bound": "hbm", "achieved": round((8.0 * Cn * rows + nb) / (ms * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBPS,
                                 "unit": "GB/s", "frac": round((8.0 * Cn * rows + nb) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 6)},
                    "logaddexp_per_s": round(evals / (ms * 1e-3), 1),
                    "logaddexp_frac_of_peak": round(evals / (ms * 1e-3) / lae_peak.value, 5) if lae_peak.value > 0 else None,
                    "parity_check": check}

        n2 = min(1000, P)
        sec["config2_beam1d_1k_reads_W10"] = beam1d_config(d_y1, d_o1, n2, Cc, int(o1[n2]), mr1, "ctc", 10, "config2")
        # the same search with the device full (every read 1 of the workload): config 2's 1 000 reads are one wave per SIMD,
        # latency-bound by construction; this is the throughput figure
        sec["beam1d_%dk_reads_W10" % (P // 1000)] = beam1d_config(d_y1, d_o1, P, Cc, tr1, mr1, "ctc", 10, "config2")
        yff, off_ff, Cff = pack_rows(ff_reads)
        d_yff, d_off_ff = torch.from_numpy(yff).to(dev), torch.from_numpy(off_ff).to(dev)
        sec["config5_flipflop_1k_reads_W10"] = beam1d_config(d_yff, d_off_ff, len(ff_reads), Cff, int(off_ff[-1]),
                                                             int(np.diff(off_ff).max()), "ctc_flipflop", 10, "config5")
        del d_yff, yff
        # config 3: one pair, latency of the whole chain (median of 5)
        wsb1 = lib.po_pair_decode_workspace_bytes(1, int(o1[1]), int(o2[1]), int(o1[1]), int(o2[1]), Cc, C.byref(opt))
        lat = timed(lambda: _lib.check(lib.po_pair_decode_batch(
            d_y1.data_ptr(), d_o1.data_ptr(), d_y2.data_ptr(), d_o2.data_ptr(), 1, Cc, C.byref(opt), d_seq1d.data_ptr(),
            d_s1o.data_ptr(), d_l1.data_ptr(), d_l2.data_ptr(), d_id.data_ptr(), d_env.data_ptr(), d_seq.data_ptr(),
            d_so.data_ptr(), d_len.data_ptr(), d_st.data_ptr(), d_ws.data_ptr(), wsb1, stream), "po_pair_decode_batch"), reps=5)
        sec["config3_single_pair_latency_ms"] = round(lat, 3)
        # the other pair-decode configurations the engine serves, same resident inputs, whole chain,
        # median of 3 launches by HIP events: Bonito's tree model, method "row", and W = 10 (the two-pairs-per-wave kernel)
        def pair_config(model, method, W, n, dy1=None, do1=None, dy2=None, do2=None, h1=None, h2=None, Cn=None, digest_key=""):
            dy1 = d_y1 if dy1 is None else dy1; do1 = d_o1 if do1 is None else do1
            dy2 = d_y2 if dy2 is None else dy2; do2 = d_o2 if do2 is None else do2
            h1 = o1 if h1 is None else h1; h2 = o2 if h2 is None else h2
            Cn = Cc if Cn is None else Cn
            q1, q2 = np.diff(h1[:n + 1]), np.diff(h2[:n + 1])
            xs1 = np.zeros(2 * n + 1, dtype=np.int64)
            cp = np.empty(2 * n, dtype=np.int64)
            cp[0::2], cp[1::2] = q1, q2
            np.cumsum(cp, out=xs1[1:])
            xso = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(q1 + q2, out=xso[1:])
            t_s1o, t_so = torch.from_numpy(xs1).to(dev), torch.from_numpy(xso).to(dev)
            t_seq1d = torch.empty(int(xs1[-1]), dtype=torch.uint8, device=dev)
            t_seq = torch.empty(int(xso[-1]), dtype=torch.uint8, device=dev)
            t_l1, t_l2, t_len, t_st = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4))
            t_id = torch.zeros(n, dtype=torch.float64, device=dev)
            t_env = torch.zeros(2 * int(h1[n]), dtype=torch.int32, device=dev)
            o = _lib.PairOptions(W, _lib.MODELS[model], _lib.METHODS[method], 5, 0, 0, 50)
            wsz = lib.po_pair_decode_workspace_bytes(n, int(h1[n]), int(h2[n]), int(q1.max()), int(q2.max()), Cn, C.byref(o))
            d_w = torch.empty(wsz, dtype=torch.uint8, device=dev)
            def launch():
                _lib.check(lib.po_pair_decode_batch(
                    dy1.data_ptr(), do1.data_ptr(), dy2.data_ptr(), do2.data_ptr(), n, Cn, C.byref(o), t_seq1d.data_ptr(),
                    t_s1o.data_ptr(), t_l1.data_ptr(), t_l2.data_ptr(), t_id.data_ptr(), t_env.data_ptr(), t_seq.data_ptr(),
                    t_so.data_ptr(), t_len.data_ptr(), t_st.data_ptr(), d_w.data_ptr(), wsz, stream), "po_pair_decode_batch")
            launch()   # (the first launch of a tree model / lane layout makes its slice pool: not part of the figures below)
            torch.cuda.synchronize()
            lib.po_profile_enable(1); lib.po_profile_reset()
            ms = timed(launch)
            torch.cuda.synchronize()
            kms, kn, mms, mn = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
            lib.po_profile_get(_lib.K_BEAM2D, C.byref(kms), C.byref(kn))
            lib.po_profile_get(_lib.K_BEAM2D_MAIN, C.byref(mms), C.byref(mn))
            lib.po_profile_enable(0)
            h_st = t_st.cpu().numpy()
            okp = int((h_st == 0).sum())
            nbs = int(t_len[t_st == 0].sum().item())
            # update_prob evaluations executed by one more launch (the counting instantiation, outside the timed ones)
            d_up = torch.zeros(2, dtype=torch.int64, device=dev)
            lib.po_profile_update_counter(d_up.data_ptr())
            _lib.check(lib.po_pair_decode_batch(
                dy1.data_ptr(), do1.data_ptr(), dy2.data_ptr(), do2.data_ptr(), n, Cn, C.byref(o), t_seq1d.data_ptr(),
                t_s1o.data_ptr(), t_l1.data_ptr(), t_l2.data_ptr(), t_id.data_ptr(), t_env.data_ptr(), t_seq.data_ptr(),
                t_so.data_ptr(), t_len.data_ptr(), t_st.data_ptr(), d_w.data_ptr(), wsz, stream), "po_pair_decode_batch")
            torch.cuda.synchronize()
            lib.po_profile_update_counter(None)
            ev_ref, ev_exe = (int(x) for x in d_up.cpu().tolist())
            lpu = {"ctc": 1, "ctc_merge_repeats": 2, "ctc_flipflop": 3}[model]   # logaddexp per update_prob (po_device.h::po_update)
            main_ms = mms.value / max(mn.value, 1)
            # strings against the oracle's digests for the same pairs, and every status named
            check = {"checked": 0, "mismatches": 0, "statuses": _status_counts(h_st),
                     "status_names": {"0": "decoded", str(_lib.SKIP_LENGTH): "skipped: basecall lengths differ by more than 1000 (pair_decode.py:331)",
                                      str(_lib.SKIP_IDENTITY): "skipped: alignment identity below 0.5 (pair_decode.py:382)",
                                      "-2": "refused as the reference refuses it: its assertion that the frame map has one entry per base fails "
                                            "(pair_decode.py:379; Bonito's get_sequence_mapping compares frame 0 with path[-1]) - the oracle returns the same code"}}
            if digest_key in sec_dig:
                want = sec_dig[digest_key]
                kk = min(n, len(want))
                h_sq = t_seq[: int(xso[kk])].cpu().numpy().tobytes()
                h_s1 = t_seq1d[: int(xs1[2 * kk])].cpu().numpy().tobytes()
                hl1, hl2, hln = t_l1[:kk].cpu().numpy(), t_l2[:kk].cpu().numpy(), t_len[:kk].cpu().numpy()
                badd = 0
                for i in range(kk):
                    stx = int(h_st[i])
                    if stx in (0, _lib.SKIP_LENGTH, _lib.SKIP_IDENTITY):
                        a_ = h_s1[xs1[2 * i]: xs1[2 * i] + hl1[i]].decode()
                        b_ = h_s1[xs1[2 * i + 1]: xs1[2 * i + 1] + hl2[i]].decode()
                        c_ = h_sq[xso[i]: xso[i] + hln[i]].decode() if stx == 0 else ""
                        got = [stx, len(a_), len(b_), len(c_), _md5(a_, b_, c_)]
                    else:   # (an engine refusal: the oracle records the same code with empty strings)
                        got = [stx, 0, 0, 0, _md5("", "", "")]
                    if got != want[i]:
                        badd += 1
                check["checked"] = kk; check["mismatches"] = badd
                if badd:   # (bit-identical by construction: no budget — see parity_check above)
                    raise SystemExit("bench.py: %s: %d of %d pairs differ from the oracle's digests" % (digest_key, badd, kk))
            return {"pairs": n, "model": model, "method": method, "beam_width": W, "chain_ms": round(ms, 3),
                    "pair_beam_stage_ms": round(kms.value / max(kn.value, 1), 3), "pair_beam_kernel_ms": round(main_ms, 3),
                    "pairs_per_s": round(n / ms * 1e3, 1), "mbases_per_s": round(nbs / ms / 1e3, 3), "decoded": okp,
                    "logaddexp_executed": ev_exe * lpu, "logaddexp_reference_schedule": ev_ref * lpu,
                    "logaddexp_frac_of_peak": round(ev_exe * lpu / (main_ms * 1e-3) / lae_peak.value, 5) if (lae_peak.value > 0 and main_ms > 0) else None,
                    "parity_check": check}
        sec["pair_bonito_W5"] = pair_config("ctc_merge_repeats", "row_col", 5, P, digest_key="pair_bonito_W5")
        sec["pair_row_W5"] = pair_config("ctc", "row", 5, P, digest_key="pair_row_W5")
        sec["pair_row_col_W10"] = pair_config("ctc", "row_col", 10, P, digest_key="pair_row_col_W10")
        # the literal defaults of the Python API (decoding_cpp.pyx:107: beam_width_ = 25, method_ = "row") and row_col at that
        # width: beam2d_kernel<., 25> (256-thread workgroups, element tables in LDS) — round 6, untimed before
        sec["pair_row_W25"] = pair_config("ctc", "row", 25, P, digest_key="pair_row_W25")
        sec["pair_row_col_W25"] = pair_config("ctc", "row_col", 25, P, digest_key="pair_row_col_W25")
        if ff_pairs is not None:
            yf1, of1, Cf = pack_rows([q[0] for q in ff_pairs])
            yf2, of2, _ = pack_rows([q[1] for q in ff_pairs])
            sec["pair_flipflop_W5"] = pair_config("ctc_flipflop", "row_col", 5, len(ff_pairs), torch.from_numpy(yf1).to(dev),
                                                  torch.from_numpy(of1).to(dev), torch.from_numpy(yf2).to(dev),
                                                  torch.from_numpy(of2).to(dev), of1, of2, Cf, digest_key="pair_flipflop_W5")
            del yf1, yf2
        torch.cuda.empty_cache()

    # whole-job aggregate: max time over ranks, sum of units
    tmax, (tot_pairs, tot_bases) = podist.job_aggregate(dist, elapsed, [Pl * args.steps, bases * args.steps], dev)

    def kernel_ms(k):
        return prof[k]

    if rank == 0:
        out = {
            "metric": "decoded Mbases/s + read-pairs/s, 10k synthetic pairs T~4000, 1/2/4/8 MI355X",
            "value": round(tot_pairs / tmax, 3),
            "unit": "read-pairs/s",
            "mbases_per_s": round(tot_bases / tmax / 1e6, 4),
            "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(tmax / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "pair-decode (Viterbi x2 + banded NW + envelope + pair beam row_col) of ONE job of %d "
                                   "synthetic pairs%s, T~%d, C=5, beam_width=%d, padding=5; inputs resident in "
                                   "HBM" % (P, "" if world == 1 else " split over %d GPUs (%d per GPU)" % (world, Pl), T, args.beam_width),
                       "pairs_per_job": P, "pairs_per_gpu": Pl, "T": T, "beam_width": args.beam_width, "method": "row_col",
                       "decoded_pairs_rank0": decoded, "parallelism": "shard%d (no collective)" % args.gpus},
        }
        if args.full:
            # algorithmic bytes per launch of the dominant kernel (pair beam search), SURVEY.md §8(d):
            # 8*C*(U+V) log-probs + 8*U envelope + L output characters, summed over the launch's pairs
            alg_bytes = 8.0 * Cc * (tr1 + tr2) + 8.0 * tr1 + bases
            b2_ms, b2_n = kernel_ms(_lib.K_BEAM2D)
            vt_ms, vt_n = kernel_ms(_lib.K_VITERBI)
            al_ms, al_n = kernel_ms(_lib.K_ALIGN)
            b2_avg = b2_ms / max(b2_n, 1)               # the stage: pre-pass + walk + store memset + kernel + deferred pass
            bk_ms, bk_n = kernel_ms(_lib.K_BEAM2D_MAIN)  # the dominant kernel alone (HIP events around its launch)
            bk_avg = bk_ms / max(bk_n, 1)
            achieved = alg_bytes / (bk_avg * 1e-3) / 1e9 if bk_avg > 0 else 0.0
            n1d = int(d_l1.sum().item() + d_l2.sum().item())
            vt_bytes = 8.0 * Cc * (tr1 + tr2) + 5.0 * n1d  # log-probs in; per base one character + one int32 frame index out
            vt_avg = vt_ms / max(vt_n, 1)
            # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process, so this figure is
            # NOT measured in this run — it comes from the newest committed rocprofv3 counter passes (profiles/
            # rNN_pmc_hbm*.json: FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, separate --pmc passes, same T / W), scaled
            # from that run's pairs per launch to this launch's
            traffic, traffic_src = None, None
            try:
                import glob
                pdir = os.path.join(REPO, "profiles")
                cands = []
                for pj in glob.glob(os.path.join(pdir, "r*_pmc_hbm*.json")):
                    with open(pj) as f:
                        pm = json.load(f)
                    kks = [v for k, v in pm.get("kernels", {}).items() if k.startswith(MAIN_KERNEL)]
                    if not kks or not (T == 4000 and args.beam_width == 5):
                        continue
                    per_launch = float(pm.get("pairs_per_launch", 1250))
                    rnd = os.path.basename(pj).split("_")[0]
                    # newest round first, then the pass whose pairs per launch is closest to this run's (traffic per pair
                    # grows with the launch size: 34 x the algorithmic bytes at 1 250 pairs per launch, 43 x at 10 000)
                    cands.append((rnd, -abs(per_launch - Pl), pj, kks[0], per_launch))
                if cands:
                    rnd, _, pj, kk, per_launch = sorted(cands, key=lambda c: (c[0], c[1]), reverse=True)[0]
                    per_pair = (2.0 * kk["FETCH_SIZE_KB_per_launch"] + kk["WRITE_SIZE_KB_per_launch"]) * 1024.0 / per_launch
                    traffic = per_pair * Pl
                    traffic_src = ("NOT measured in this run: %s (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes at %d "
                                   "pairs per launch; FETCH_SIZE x 2 on gfx950), scaled by pairs" % (os.path.relpath(pj, REPO), int(per_launch)))
            except Exception:
                pass
            out.update({
                "roofline": {"bound": "hbm", "kernel": MAIN_KERNEL + (", true>" if LEGACY else ""), "achieved": round(achieved, 3),
                             "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBPS, 6),
                             "traffic": traffic, "traffic_source": traffic_src, "alg_bytes_per_launch": alg_bytes, "avg_launch_ms": round(bk_avg, 3),
                             "launches": bk_n, "stage_ms": round(b2_avg, 3),
                             "note": "f64 log-space beam search: bound by the f64 instruction stream of logaddexp and "
                                     "per-step bookkeeping latency, not by HBM (SURVEY.md §8(d), DESIGN.md §3.3); the "
                                     "streaming Viterbi kernel is the HBM-bound one, see viterbi_roofline"},
                "viterbi_roofline": {"bound": "hbm", "kernel": "viterbi_ctc_kernel (2 launches per step)",
                                     "achieved": round(vt_bytes / (vt_avg * 1e-3) / 1e9, 3) if vt_avg > 0 else 0.0,
                                     "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                     "frac": round(vt_bytes / (vt_avg * 1e-3) / 1e9 / HBM_PEAK_GBPS, 6) if vt_avg > 0 else 0.0,
                                     "avg_ms_per_step": round(vt_avg, 3)},
                "stage_ms_per_step": {"viterbi_x2": round(vt_avg, 3), "align_envelope": round(al_ms / max(al_n, 1), 3),
                                      "pair_beam": round(b2_avg, 3)},
            })
            # the pair beam search priced against what actually bounds it: one logaddexp per update_prob (ctc)
            lae_rate = n_upd / (bk_ms * 1e-3) if bk_ms > 0 else 0.0   # (kernel time, like `roofline`)
            exe_rate = n_upd_exec / (bk_ms * 1e-3) if bk_ms > 0 else 0.0
            out["compute_roofline"] = {"bound": "f64 logaddexp stream (VALU)", "unit": "logaddexp/s",
                                       "achieved": round(exe_rate, 1), "peak": round(lae_peak.value, 1),
                                       "frac": round(exe_rate / lae_peak.value, 5) if lae_peak.value > 0 else None,
                                       "executed_per_step": n_upd_exec // max(args.steps, 1),
                                       "reference_schedule_per_step": n_upd // max(args.steps, 1),
                                       "reference_schedule_frac": round(lae_rate / lae_peak.value, 5) if lae_peak.value > 0 else None,
                                       "note": "achieved / frac = update_prob evaluations the pair beam kernel EXECUTES / its "
                                               "time, against the po_lae_peak micro-benchmark on this device (all lanes busy, 4 "
                                               "independent chains per lane, same table-driven logaddexp); "
                                               "reference_schedule_* counts what the reference's schedule evaluates for this "
                                               "input (every element over its full windows in every step) — the kernel skips "
                                               "the ones whose result is provably already stored (bit-identical output).  "
                                               "beam2d_reg_kernel (round 4) executes about HALF of what round 3's "
                                               "beam2d_kernel did on the same pairs (3.6e9 against 7.3e9 per 10 000 pairs: "
                                               "continuing elements compute new times only), so `frac` fell while the kernel "
                                               "got faster; reference_schedule_frac compares like with like across rounds"}
        if weak is not None:
            out["weak_scaling"] = weak
        if parity is not None:
            out["parity_check"] = parity
        if sec:
            out["secondary"] = sec
        if two_streams is not None:
            out["two_streams"] = two_streams
        if strong is not None:
            out["strong_scaling"] = strong
            if world == 1:
                out["e2e_pairs_per_s"] = strong["pairs_per_s"]
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
            out["gpu_over_cpu_all_cores"] = round(out["value"] / cpu_base["value"], 1)
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
