"""Flagship benchmark: test-input prioritization throughput on MI355X.

Measures the BASELINE.json headline metric — inputs/sec prioritized
(activation-trace extraction + LSA + DSA + DeepGini scoring) on the
CIFAR-10 ResNet-20 config — on synthetic data / random-init weights.

One timed step = prioritize a fresh per-GPU batch of test inputs:
  1. forward with AT taps (bf16 autocast, tap = 4096-wide stage-3 feature map)
  2. DeepGini & softmax-family scores (fused HIP epilogue)
  3. DSA against the 0.3-subsampled train ATs (MFMA pairwise rowmin, two-hop)
  4. per-class LSA (whitened MFMA pairwise + logsumexp epilogue)
  5. all-gather of the per-input score shards over RCCL/xGMI (world > 1)
Setup (train-AT extraction, KDE/covariance fits) is untimed, mirroring the
reference's [setup, pred, quant] timing taxonomy (eval_apfd_table.py:176-232).

Scaling is WEAK: each GPU prioritizes its own fixed-size test shard against
the full (replicated) train-AT set.

Usage: python bench.py --gpus N --steps K --warmup W [--batch B]
                       [--dump-outputs DIR] [--full]
(the driver launches N>1 via torch.distributed.run, one rank per GPU).

A plain run does only what the headline figure needs: setup, warm-up, the
K timed steps, the result line. --dump-outputs DIR additionally writes the
scores the last timed step returned (DIR/<name>.npy, float32) so two builds
can be compared output for output: with the same arguments every input
(weights, train ATs, test batches) is identical from run to run. --full adds
the auxiliary quality signals (last-batch APFDs and the deep-gini nominal
APFD pin), which a plain run leaves out of the result line's config (null).
"""

import argparse
import concurrent.futures
import json
import os
import sys
import time

_T_START = time.perf_counter()  # log() stamps are seconds since process start

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from simple_tip_amd import ops
from simple_tip_amd.core.apfd import apfd_from_order
from simple_tip_amd.core.surprise import DSA, LSA, MultiModalSA
from simple_tip_amd.models import ResNet20
from simple_tip_amd.parallel import dist as pdist

TRAIN_N = 50000
AT_TAP = ResNet20.sa_layers  # layer 9: 8x8x64 = 4096-wide feature map


def log(rank, msg):
    if rank == 0:
        print(f"[bench] +{time.perf_counter() - _T_START:5.1f}s {msg}",
              file=sys.stderr, flush=True)


class GraphedExtractor:
    """Inference-path AT extractor: BN-folded bf16 channels_last model,
    fixed-shape forward captured in a hipGraph (one replay per step).

    Motivated by profiles/r01_bench_kernels.md: BN-inference launches and
    small-conv launch overhead dominated the step before this.
    """

    def __init__(self, model, batch, device, use_graph=True):
        from simple_tip_amd.models.fuse import fold_bn_inference, pad_stem_channels

        self.device = device
        self.batch = batch
        m = fold_bn_inference(model).to(device)
        self.in_ch = 3
        self.fused = None
        if device.type == "cuda" and os.environ.get("TIP_NO_FUSED_RESNET") != "1":
            try:
                from simple_tip_amd.models.resnet_fused import FusedResNet20

                self.fused = FusedResNet20(m, device)
            except Exception as e:  # pragma: no cover
                print(f"[bench] fused ResNet path unavailable ({e!r})",
                      file=sys.stderr)
        if device.type == "cuda":
            pad_stem_channels(m, 4)  # NHWC bf16 igemm path needs >=4 channels
            self.in_ch = 4
            self.model = m.to(torch.bfloat16).to(memory_format=torch.channels_last)
        else:
            self.model = m
        self.graph = None
        self.fused_graph = None
        if use_graph and device.type == "cuda":
            try:
                if self.fused is not None:
                    self._capture_fused()
                else:
                    self._capture()
            except Exception as e:  # pragma: no cover - graph capture optional
                print(f"[bench] hipGraph capture failed ({e!r}); eager path",
                      file=sys.stderr)
                self.graph = None
                self.fused_graph = None

    @torch.no_grad()
    def _capture_fused(self):
        """Capture the whole fused forward (channel pad + 11 block kernels +
        pool/fc + softmax) into one hipGraph replay. Input is NHWC fp32."""
        self.fstatic_x = torch.zeros(self.batch, 32, 32, 3, device=self.device)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.fused.forward_nhwc(self.fstatic_x)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ats, logits = self.fused.forward_nhwc(self.fstatic_x)
            self.fstatic_ats = ats
            self.fstatic_probs = torch.softmax(logits, dim=1)
        self.fused_graph = g

    @torch.no_grad()
    def _capture(self):
        self.static_x = torch.zeros(
            self.batch, self.in_ch, 32, 32, device=self.device,
            dtype=torch.bfloat16,
        ).to(memory_format=torch.channels_last)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):  # warm up MIOpen finds before capture
                self.model.forward_taps(self.static_x, AT_TAP)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            taps, logits = self.model.forward_taps(self.static_x, AT_TAP)
            self.static_at = taps[0]
            self.static_logits = logits
        self.graph = g

    def _prep(self, x):
        xb = x.to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            xb = xb.to(torch.bfloat16)
            if self.in_ch > xb.shape[1]:
                pad = torch.zeros(
                    xb.shape[0], self.in_ch - xb.shape[1], *xb.shape[2:],
                    dtype=xb.dtype, device=xb.device,
                )
                xb = torch.cat([xb, pad], dim=1)
            xb = xb.to(memory_format=torch.channels_last)
        return xb

    @torch.no_grad()
    def __call__(self, x):
        if self.fused is not None:
            is_nhwc = x.dim() == 4 and x.shape[-1] == 3
            if (
                self.fused_graph is not None
                and is_nhwc
                and x.shape[0] == self.batch
            ):
                self.fstatic_x.copy_(x.to(self.device, torch.float32))
                self.fused_graph.replay()
                return self.fstatic_ats, self.fstatic_probs
            ats, logits = (
                self.fused.forward_nhwc(x) if is_nhwc else self.fused(x)
            )
            return ats, torch.softmax(logits, dim=1)
        if self.graph is not None and x.shape[0] == self.batch:
            self.static_x.copy_(self._prep(x))
            self.graph.replay()
            at = self.static_at
            logits = self.static_logits
        else:
            taps, logits = self.model.forward_taps(self._prep(x), AT_TAP)
            at = taps[0]
        ats = at.reshape(at.shape[0], -1).float()
        probs = torch.softmax(logits.float(), dim=1)
        return ats, probs


def dump_outputs(out_dir, last):
    """Write what the last timed step returned to its caller — the deep-gini,
    DSA and per-class LSA scores and the (remapped) predicted classes of that
    step's batch — as out_dir/<name>.npy, float32, one value per input."""
    os.makedirs(out_dir, exist_ok=True)
    names = ("deep_gini", "dsa", "pc_lsa", "pred")
    for name, t in zip(names, last):
        if t is None:
            continue
        arr = torch.as_tensor(t).detach().float().cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), arr.astype(np.float32))


QUALITY_KEYS = (
    "apfd_gini_lastbatch",
    "apfd_gini_nominal_lastbatch",
    "apfd_dsa_lastbatch",
    "apfd_pclsa_lastbatch",
)


def quality_signals(rank, last, last_labels, batch):
    """--full only: APFD of each scorer's ordering on the last timed batch,
    and the deep-gini nominal-half pin. Returns the config entries (None
    where an APFD is undefined)."""
    gini, dsa_last, lsa_last, pred = last
    mis = (pred.cpu().numpy() != last_labels.numpy())

    def _apfd(scores):
        if not mis.any():
            return float("nan")
        return apfd_from_order(
            mis, np.argsort(-scores.float().cpu().numpy(), kind="stable")
        )

    apfd = _apfd(gini)
    apfd_dsa = _apfd(dsa_last)
    apfd_lsa = _apfd(lsa_last) if lsa_last is not None else float("nan")
    # quality pin: on the NOMINAL half of the batch a
    # trained model's deep-gini ordering must beat random — rules out a
    # sign/negation bug producing a plausible-looking throughput number
    half = batch // 2
    mis_nom = mis[:half]
    apfd_gini_nom = float("nan")
    if mis_nom.sum() >= 10:
        apfd_gini_nom = apfd_from_order(
            mis_nom,
            np.argsort(-gini[:half].float().cpu().numpy(), kind="stable"),
        )
        # assert only on statistically meaningful configs: a large nominal
        # half and a model that actually learned (tiny smoke configs train
        # for seconds and gini on a near-random model IS near-random)
        if half >= 2000 and mis_nom.mean() < 0.5:
            assert apfd_gini_nom > 0.5, (
                f"deep-gini nominal APFD {apfd_gini_nom:.3f} <= 0.5: softmax "
                f"ordering is not ranking real faults"
            )
    log(rank, f"last-batch accuracy={1.0 - mis.mean():.3f} "
              f"apfd_gini={apfd:.3f} apfd_gini_nominal={apfd_gini_nom:.3f} "
              f"apfd_dsa={apfd_dsa:.3f} apfd_lsa={apfd_lsa:.3f}")
    values = (apfd, apfd_gini_nom, apfd_dsa, apfd_lsa)
    return {
        k: None if np.isnan(v) else v for k, v in zip(QUALITY_KEYS, values)
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=20480,
                    help="test inputs per GPU per step (default = the reference's\n                    OOD test-set size; larger batches amortize per-step overhead)")
    ap.add_argument("--train-n", type=int, default=TRAIN_N)
    ap.add_argument("--setup-epochs", type=int, default=1,
                    help="untimed warm-up training epochs (class diversity); "
                         "one epoch is 80 Adam steps of 128 inputs")
    ap.add_argument("--shard-train", action="store_true",
                    help="strong scaling: shard the train-AT axis across "
                         "ranks; every rank scores the SAME batch against "
                         "its shard, partials merge over RCCL")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the scores the last "
                         "timed step returned as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also compute the auxiliary quality signals "
                         "(last-batch APFDs, deep-gini nominal APFD pin)")
    args = ap.parse_args()

    rank, world, device = pdist.init_from_env()
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != env_world:
        raise SystemExit(
            f"--gpus {args.gpus} but WORLD_SIZE={env_world}: for N>1 launch "
            f"via `python -m torch.distributed.run --nnodes=1 "
            f"--nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N`"
        )
    on_gpu = device.type == "cuda"
    # note: torch.backends.cudnn.benchmark=True was measured WORSE here
    # (forward 16.4 -> 72.3 ms; MIOpen's "benchmark" find picked slower
    # algos for these NHWC bf16 shapes) — keep the default heuristic find.
    if on_gpu and not ops.hip_available():
        raise RuntimeError("bench on GPU requires the _tip_hip extension")

    torch.manual_seed(0)  # identical weights on every rank
    model = ResNet20().eval()  # trained on the host below, then moved

    # ---- setup (untimed) ----
    # Brief training on class-structured synthetic data so the model's
    # predictions spread over all classes: a random-init net predicts one
    # class for everything, which would degenerate the per-class DSA/LSA
    # work in the timed region (work-skipping = invalid measurement).
    from simple_tip_amd.studies.synthetic import corrupt_images, synthetic_images

    # Host-side synthetic data. Every array is seeded by its (study, split)
    # name alone, so generating the splits on worker threads (numpy releases
    # the GIL) during the warm-up training changes no value, only the setup's
    # wall time: serially this was about half of a plain run.
    shard_train = bool(args.shard_train) and world > 1
    n_pool = min(max(args.steps + args.warmup, 4), 8)

    def gen_split(split, n):
        return synthetic_images("bench_cifar10", split, n, (3, 32, 32), 10)

    def gen_test_batch(i):
        # shard-train mode: every rank scores the SAME global batch (strong
        # scaling), so the pool seed must not depend on rank
        tag = f"test-shared-{i}" if shard_train else f"test-r{rank}-{i}"
        px, py = gen_split(tag, args.batch)
        # reference OOD recipe: half the batch is corrupted, so the model
        # has real faults for the APFD quality signal
        half = args.batch // 2
        px[half:] = corrupt_images("bench_cifar10", px[half:], severity=0.5)
        return px, py

    datagen = concurrent.futures.ThreadPoolExecutor(max_workers=6)
    warm_f = datagen.submit(gen_split, "warm", 10240)
    train_f = datagen.submit(gen_split, "train", args.train_n)
    pool_f = [datagen.submit(gen_test_batch, i) for i in range(n_pool)]
    datagen.shutdown(wait=False)

    tx, ty = warm_f.result()
    tx_t = torch.from_numpy(tx)
    ty_t = torch.from_numpy(ty)
    opt = torch.optim.Adam(model.parameters(), lr=2e-3)
    model.train()
    # The warm-up runs on the host in fp32, whatever the device. On the GPU
    # it went through MIOpen, whose backward solvers accumulate with atomics
    # (weights, train ATs and so every score differed from run to run, the
    # predicted-class histogram by 10x) and whose kernels compile at first
    # use (~14 s with an empty cache); its deterministic solvers cost 0.2 s
    # a step on top. An epoch of 80 steps of 128 on the host takes a few
    # seconds and gives identical weights every run on every build. Keep
    # the step count: after 20 steps (of 512) the BN running statistics had
    # not converged and the eval-mode net predicted one or two classes.
    log(rank, f"warm-up training x{args.setup_epochs} epochs (host)")
    for epoch in range(args.setup_epochs):
        perm = torch.randperm(tx_t.shape[0])
        for s in range(0, tx_t.shape[0], 128):
            idx = perm[s : s + 128]
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(model(tx_t[idx]), ty_t[idx])
            loss.backward()
            opt.step()
    model.eval().to(device)
    if world > 1:
        # correctness by construction: rank-0 weights everywhere
        for p in model.parameters():
            torch.distributed.broadcast(p.data, src=0)

    # train-AT extraction + SA fits (the reference's "setup" bucket)
    base_x, base_y = train_f.result()
    train_x = torch.from_numpy(base_x)
    # in shard-train mode each rank forwards only its slice of the batch, so
    # the hipGraph is captured at the slice size
    if args.shard_train and world > 1:
        _sl0 = pdist.shard_slice(args.batch)
        cap_batch = _sl0.stop - _sl0.start
    else:
        cap_batch = args.batch
    extractor = GraphedExtractor(model, cap_batch, device, use_graph=on_gpu)

    if shard_train:
        # each rank extracts ATs for its row shard, then the full train-AT
        # tensor all-gathers (one-time, untimed setup) so SA fits are
        # identical everywhere; DSA/LSA then keep only their row shards.
        my_rows = train_x[pdist.shard_slice(args.train_n)]
    else:
        my_rows = train_x
    log(rank, f"extracting train ATs ({my_rows.shape[0]} x 4096)")
    at_parts, pred_parts = [], []
    for s in range(0, my_rows.shape[0], 1024):
        a, p = extractor(my_rows[s : s + 1024])
        at_parts.append(a.float())  # SA fits are fp32 (setup, untimed)
        pred_parts.append(p.argmax(dim=1))
    train_ats = torch.cat(at_parts)
    train_pred = torch.cat(pred_parts)
    if shard_train:
        train_ats = pdist.allgather_rows(train_ats, args.train_n)
        train_pred = pdist.allgather_rows(train_pred, args.train_n)
    del train_x, my_rows, at_parts, pred_parts
    if torch.unique(train_pred).numel() < 2:
        # last-resort guard (should not trigger after warm-up training):
        # use the synthetic labels so the per-class SA work is real
        log(rank, "WARNING: predictions collapsed; using labels for SA fit")
        train_pred = torch.from_numpy(base_y).to(train_pred.device)

    log(rank, f"train pred classes: {torch.bincount(train_pred.cpu(), minlength=10).tolist()}")
    log(rank, "fitting DSA (0.3 subsample) + per-class LSA"
              + (" [train axis sharded]" if shard_train else ""))
    dsa = DSA(
        train_ats, train_pred, subsampling=0.3, device=device,
        shard_train=shard_train,
    )
    lsa = MultiModalSA.build_by_class(
        train_ats, train_pred,
        lambda a, p: LSA(a, max_features=300, device=device,
                         shard_train=shard_train),
    )
    train_classes = set(torch.unique(train_pred.cpu()).tolist())

    fused_prio = None
    if on_gpu and os.environ.get("TIP_NO_FUSED_PRIO") != "1":
        try:
            from simple_tip_amd.engine.serving import FusedPrioritizer

            # bf16 pairwise kernels by default (the bench's declared compute
            # dtype is bf16; TIP_FP32_PAIRWISE=1 restores the fp32 MFMA path)
            pdtype = (
                None if os.environ.get("TIP_FP32_PAIRWISE") == "1"
                else torch.bfloat16
            )
            fused_prio = FusedPrioritizer(dsa, lsa, device, pairwise_dtype=pdtype)
            log(rank, f"fused prioritizer ready (lsa={fused_prio.lsa_ready}, "
                      f"bf16={fused_prio.bf16})")
        except Exception as e:  # pragma: no cover
            log(rank, f"fused prioritizer unavailable: {e!r}")

    # pre-generate per-rank test batches (distinct per step and rank, same
    # class-structured distribution as training so predictions spread).
    # Default: batches are staged into HBM during (untimed) setup — 8 pool
    # slots x 125 MB is 1 GB of the 288 GB, and the 125 MB/step PCIe H2D
    # otherwise becomes the critical path (measured ~2 ms/step stall even
    # with a dedicated prefetch stream). TIP_HOST_POOL=1 restores pinned-
    # host batches with double-buffered prefetch for the streaming story.
    host_pool = os.environ.get("TIP_HOST_POOL") == "1"
    log(rank, f"staging {n_pool} test batches")
    pool, labels_pool = [], []
    nhwc_pool = extractor.fused is not None
    for i in range(n_pool):
        px, py = pool_f[i].result()
        pool_f[i] = None
        t = torch.from_numpy(px)
        if nhwc_pool:
            t = t.permute(0, 2, 3, 1).contiguous()
        if on_gpu:
            t = t.pin_memory() if host_pool else t.to(device)
        pool.append(t)
        labels_pool.append(torch.from_numpy(py))

    if on_gpu and not host_pool:
        # HBM-resident pool: no prefetch machinery needed
        def prefetch(i):
            pass

        def get_batch(i):
            return pool[i % len(pool)]

        def mark_consumed(i):
            pass
    elif on_gpu:
        copy_stream = torch.cuda.Stream()
        buf_shape = (
            (args.batch, 32, 32, 3) if nhwc_pool else (args.batch, 3, 32, 32)
        )
        dev_bufs = [torch.empty(*buf_shape, device=device) for _ in range(2)]
        copy_events = [torch.cuda.Event(), torch.cuda.Event()]
        consumed_events = [torch.cuda.Event(), torch.cuda.Event()]

        def prefetch(i):
            with torch.cuda.stream(copy_stream):
                # don't overwrite the buffer until the step that read it has
                # been fully enqueued ahead of us on the compute stream
                copy_stream.wait_event(consumed_events[i % 2])
                dev_bufs[i % 2].copy_(pool[i % len(pool)], non_blocking=True)
                copy_events[i % 2].record(copy_stream)

        def get_batch(i):
            torch.cuda.current_stream().wait_event(copy_events[i % 2])
            return dev_bufs[i % 2]

        def mark_consumed(i):
            consumed_events[i % 2].record(torch.cuda.current_stream())

        prefetch(0)
    else:
        def prefetch(i):
            pass

        def get_batch(i):
            return pool[i % len(pool)]

        def mark_consumed(i):
            pass

    phase_log = os.environ.get("TIP_BENCH_PHASES") == "1"
    seen = torch.tensor(sorted(train_classes), device=device)

    # ---- two-stage software pipeline (GPU): forward[i+1] runs on its own
    # stream while the scoring of batch i (softmax family + grouped DSA/LSA)
    # runs on the main stream. The extractor's hipGraph replay writes static
    # output buffers, so each forward's (ats, probs) are copied into parity
    # double-buffers before the next replay may clobber them; per-parity
    # events order buffer reuse. Scoring must not host-sync (the class-remap
    # guard is branch-free) or the overlap collapses.
    fwd_stream = torch.cuda.Stream() if on_gpu else None
    fwd_done = [torch.cuda.Event(), torch.cuda.Event()] if on_gpu else None
    score_done = [torch.cuda.Event(), torch.cuda.Event()] if on_gpu else None
    out_bufs = [None, None]

    def extract(x):
        """AT extraction for one global batch.

        In shard-train mode the FORWARD is sharded too: each rank extracts
        its slice of the (replicated) batch and the ats/probs all-gather,
        so every rank scores identical tensors — per-class segment sizes
        (and therefore every later collective's shape) agree across ranks
        BY CONSTRUCTION, independent of nondeterministic training/forward
        differences between ranks.
        """
        if shard_train:
            sl = pdist.shard_slice(x.shape[0])
            a_l, p_l = extractor(x[sl].contiguous())
            ats = pdist.allgather_rows(a_l.contiguous(), x.shape[0])
            probs = pdist.allgather_rows(p_l.contiguous(), x.shape[0])
            return ats, probs
        return extractor(x)

    def launch_forward(i):
        """Enqueue batch i's extraction on the forward stream."""
        p = i % 2
        with torch.cuda.stream(fwd_stream):
            fwd_stream.wait_event(score_done[p])  # buffer p free?
            x = get_batch(i)
            ats, probs = extract(x)
            mark_consumed(i)
            prefetch(i + 1)
            if out_bufs[p] is None:
                out_bufs[p] = (torch.empty_like(ats), torch.empty_like(probs))
            out_bufs[p][0].copy_(ats)
            out_bufs[p][1].copy_(probs)
            fwd_done[p].record(fwd_stream)

    def score(i):
        """Score batch i's (already extracted) activations on this stream."""
        p = i % 2
        s = torch.cuda.current_stream()
        s.wait_event(fwd_done[p])
        ats, probs = out_bufs[p]
        # branch-free synthetic-data guard: remap predictions of classes
        # unseen in training (no host sync — it would serialise the pipe)
        pred = probs.argmax(dim=1)
        pred = torch.where(torch.isin(pred, seen), pred, seen[0])
        unc = ops.softmax_uncertainties(probs)
        if fused_prio is not None and fused_prio.lsa_ready:
            dsa_scores, lsa_scores = fused_prio(ats, pred)
        else:
            dsa_scores = dsa(ats, pred)
            lsa_scores = lsa(ats, pred)
        gini = unc["deep_gini"]
        # publish score shards (tiny, latency-bound on xGMI). In shard-train
        # mode the DSA/LSA partials already merged inside the prioritizer and
        # every rank holds full-batch scores — nothing left to gather.
        if world > 1 and not shard_train:
            n_total = args.batch * world
            gini_all = pdist.allgather_rows(gini, n_total)
            dsa_all = pdist.allgather_rows(dsa_scores.float().to(device), n_total)
            _ = (gini_all, dsa_all)
        score_done[p].record(torch.cuda.current_stream())
        return gini, dsa_scores, lsa_scores, pred

    def step(i, timed_phases=False):
        """Non-pipelined step (CPU path and phase-instrumented runs)."""
        marks = []

        def mark(name):
            if timed_phases:
                # sync only the compute stream: a device-wide sync would
                # also wait for the overlapped H2D prefetch and mis-bill it
                torch.cuda.current_stream().synchronize()
                marks.append((name, time.perf_counter()))

        x = get_batch(i)
        mark("start")
        ats, probs = extract(x)
        mark_consumed(i)
        prefetch(i + 1)
        pred = probs.argmax(dim=1)
        pred = torch.where(torch.isin(pred, seen.to(pred.device)), pred, seen.to(pred.device)[0])
        mark("forward")
        unc = ops.softmax_uncertainties(probs)
        mark("unc")
        if fused_prio is not None and fused_prio.lsa_ready:
            dsa_scores, lsa_scores = fused_prio(ats, pred)
            mark("dsa+lsa")
        else:
            dsa_scores = dsa(ats, pred)
            mark("dsa")
            lsa_scores = lsa(ats, pred)
            mark("lsa")
        gini = unc["deep_gini"]
        if world > 1 and not shard_train:
            n_total = args.batch * world
            gini_all = pdist.allgather_rows(gini, n_total)
            dsa_all = pdist.allgather_rows(dsa_scores.float().to(device), n_total)
            _ = (gini_all, dsa_all)
        mark("gather")
        if timed_phases and marks:
            parts = [
                f"{marks[j][0]}={1000*(marks[j][1]-marks[j-1][1]):.1f}ms"
                for j in range(1, len(marks))
            ]
            log(rank, "phases: " + " ".join(parts))
        return gini, dsa_scores, lsa_scores, pred

    pipelined = on_gpu and os.environ.get("TIP_NO_PIPELINE") != "1"
    log(rank, f"warmup x{args.warmup} (pipelined={pipelined})")
    if pipelined:
        for i in range(args.warmup):
            launch_forward(i)
            score(i)
        if phase_log:
            torch.cuda.synchronize()
            step(args.warmup - 1, timed_phases=True)  # phase breakdown, unpipelined
    else:
        for i in range(args.warmup):
            step(i, timed_phases=phase_log and on_gpu and i == args.warmup - 1)

    pdist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        if pipelined:
            # enqueue batch i's forward, then its scoring: the host runs
            # ahead, so forward[i+1] lands on the forward stream while the
            # GPU still executes scoring[i] on the main stream
            launch_forward(args.warmup + i)
            last = score(args.warmup + i)
        else:
            last = step(args.warmup + i)
    pdist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    elapsed = pdist.allreduce_max_scalar(elapsed, device)

    per_step_inputs = args.batch if shard_train else args.batch * world
    total_inputs = per_step_inputs * args.steps
    value = total_inputs / elapsed
    ms_per_step = elapsed / args.steps * 1000.0
    log(rank, f"timed x{args.steps}: {ms_per_step:.3f} ms/step")

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last)

    quality = dict.fromkeys(QUALITY_KEYS)
    if args.full:
        last_labels = labels_pool[(args.warmup + args.steps - 1) % len(pool)]
        quality = quality_signals(rank, last, last_labels, args.batch)

    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": "inputs_per_sec_prioritized",
                    "value": value,
                    "unit": "inputs/s",
                    "n_gpus": world,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": ms_per_step,
                    "higher_is_better": True,
                    "scaling": "strong" if shard_train else "weak",
                    "vs_baseline": None,
                    "dtype": "bf16",
                    "data": "synthetic",
                    "config": {
                        "model": "cifar10_resnet20",
                        "global_batch": per_step_inputs,
                        "seq_len": None,
                        "parallelism": (
                            f"train-shard{world}" if shard_train else f"dp{world}"
                        ),
                        "train_ats": args.train_n,
                        "at_width": 4096,
                        "input_residency": (
                            "host-pinned" if os.environ.get("TIP_HOST_POOL") == "1"
                            else "hbm"
                        ),
                        "scorers": "gini+softmax-family+dsa+pc-lsa",
                        **quality,  # null unless --full
                    },
                }
            ),
            flush=True,
        )
    if pdist.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
