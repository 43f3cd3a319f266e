"""Production serving path: fused per-batch prioritization.

The generic SA classes (core/surprise.py) loop python-side over predicted
classes — fine for experiment runs, but at serving rates the ~200 host-side
torch ops per batch become the bottleneck (the GPU finishes in ~18 ms while
the host enqueues for ~35 ms; see profiles/). :class:`FusedPrioritizer`
lowers a DSA + per-class-LSA pipeline onto the grouped (segmented) pairwise
kernels: the batch is class-sorted once, padded to 128-row segments, and a
SINGLE kernel launch covers every class for DSA (and one for LSA), cutting
the host op count per batch to ~40.

In bf16 mode the sort-and-pad itself moves to the device (the sync-free path
below): a plan kernel writes the padded-row -> source-row map and the
kernels gather through it, ~10 launches per batch with no host<->device
copy, so the host can queue the next forward while a batch is still scoring.

Numerics: the fp32 mode is identical to the per-class path (same kernels,
same fp32 accumulation, same tie rules; tests/test_gpu_serving.py asserts
equality). The optional bf16 mode (``pairwise_dtype=torch.bfloat16``) uses
the bf16-operand MFMA kernels — 4.6x faster, scores shift only by operand
rounding (rank correlation > 0.99 vs fp32, pinned by test).
"""

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..core.surprise import DSA, LSA, GroupedGaussianSA, MultiModalSA
from ..ops import _load_compiled


class FusedPrioritizer:
    """Batched DSA + per-class LSA scorer on the grouped kernels (GPU).

    When the DSA (and the LSA instances) were fit with ``shard_train`` on an
    initialised torch.distributed group, the train side of the grouped
    kernels is this rank's per-class row shard: every rank scores the SAME
    (replicated) batch against 1/world of the train rows, then the partial
    (min, argmin) / logsumexp results merge with deterministic rank-ordered
    reductions over RCCL (parallel/sharded.py semantics), so sharded scores
    equal single-device ones.

    ``gaussian`` adds Gaussian scorers (pc-MDSA / pc-MLSA / pc-MMDSA as
    ``MultiModalSA`` of MDSA or MLSA modes) served by :meth:`score_all`
    through the grouped Gaussian kernels; ``__call__`` is unaffected.
    """

    def __init__(
        self,
        dsa: DSA,
        lsa: Optional[MultiModalSA],
        device,
        pairwise_dtype=None,
        fast: Optional[bool] = None,
        gaussian: Optional[Dict[str, MultiModalSA]] = None,
    ):
        self.ext = _load_compiled()
        self.device = device
        # Gaussian scorers served by score_all(): each MultiModalSA of MDSA /
        # MLSA modes is fuse()d here once. Serving follows the DSA / LSA rule
        # for ids without a fitted mode (+inf, no host check), so a call
        # stays free of device-to-host copies.
        self.gaussian: Dict[str, GroupedGaussianSA] = {}
        for name, sa in (gaussian or {}).items():
            if name in ("dsa", "pc-lsa"):
                raise ValueError(f"gaussian scorer name {name!r} is reserved")
            self.gaussian[name] = (
                sa if isinstance(sa, GroupedGaussianSA) else sa.fuse(device=device)
            )
        if dsa._class_cache is None:
            dsa._build_class_cache()
        self.num_classes = dsa.num_classes
        self.shard_train = bool(getattr(dsa, "shard_train", False))
        # bf16 pairwise path (fp32 accumulate): the ATs come out of a bf16
        # forward, so bf16 operands cost ~nothing in signal while the MFMA
        # ceiling rises ~16x over fp32. Scores shift by bf16 rounding of the
        # cross terms — the engine's parity paths stay fp32; the bench opts
        # in (its declared compute dtype is bf16).
        self.bf16 = pairwise_dtype == torch.bfloat16

        # class-concatenated DSA train side + GLOBAL b-table. In shard mode
        # the cache's `same` is the local row shard while `b_table` is the
        # full (all-gathered) per-class table, so `btableS` is identical on
        # every rank and the local→global row map sends grouped-kernel argmin
        # indices (local concatenation) to full-concatenation rows.
        trains, btables, offs = [], [], [0]
        l2g_parts = []
        g_off = 0
        for c in range(self.num_classes):
            same, b_table, _, off = dsa._class_cache[c]
            if same is None:
                offs.append(offs[-1])
                continue
            n_full = b_table.shape[0] if b_table is not None else same.shape[0]
            trains.append(same.float())
            bt = (
                b_table.float().to(device)
                if b_table is not None
                else torch.full((n_full,), float("inf"), device=device)
            )
            btables.append(bt)
            offs.append(offs[-1] + same.shape[0])
            if self.shard_train:
                l2g_parts.append(
                    g_off + off + torch.arange(
                        same.shape[0], dtype=torch.int64, device=device
                    )
                )
            g_off += n_full
        self.trainS = torch.cat(trains).contiguous().to(device)
        self.btableS = torch.cat(btables).contiguous().to(device)
        self.bnormS = (self.trainS * self.trainS).sum(dim=1).contiguous()
        if self.bf16:
            self.trainS16 = self.trainS.to(torch.bfloat16).contiguous()
            f = self.trainS16.float()
            self.bnormS16 = (f * f).sum(dim=1).contiguous()  # bf16-exact norms
            del f
        self.nseg = torch.tensor(offs, dtype=torch.int32, device=device)
        self.local2global = (
            torch.cat(l2g_parts) if self.shard_train else None
        )
        self.jb_max = max(
            1,
            max(
                (offs[c + 1] - offs[c] + 127) // 128
                for c in range(self.num_classes)
            ),
        )

        # per-class LSA state. A class is either
        #   "fused":    (keep idx, L^-T, const) + its whitened-train segment
        #   "const":    degraded KDE (reference semantics: density-0 classes
        #               score 0; prepare-failed classes score +inf)
        #   "fallback": feature count differs from the majority (drop-feature
        #               retry ladder fired) — scored via the per-class SA
        self.lsa_ready = False
        if lsa is not None:
            self.lsa_mode = []
            wtrains, woffs = [], [0]
            consts = [0.0] * self.num_classes
            d_ref = None
            any_fused = False
            for c in range(self.num_classes):
                sa = lsa.modal_sa.get(c)
                if sa is None or not isinstance(sa, LSA):
                    self.lsa_mode.append(("const", float("inf")))
                    woffs.append(woffs[-1])
                    continue
                if sa.kde is None:
                    # all features removed / singleton class: density 0
                    self.lsa_mode.append(("const", 0.0))
                    woffs.append(woffs[-1])
                    continue
                if sa.kde.prepare_failed:
                    self.lsa_mode.append(("const", float("inf")))
                    woffs.append(woffs[-1])
                    continue
                linv_t, xw, const = sa.kde.device_state(device)
                if self.shard_train:
                    from ..parallel.sharded import shard_rows

                    xw, _ = shard_rows(xw)
                if d_ref is None:
                    d_ref = linv_t.shape[0]
                if linv_t.shape[0] != d_ref:
                    self.lsa_mode.append(("fallback", sa))
                    woffs.append(woffs[-1])
                    continue
                keep = (
                    torch.from_numpy(
                        np.delete(
                            np.arange(linv_t.shape[0] + len(sa.removed_neurons)),
                            sa.removed_neurons,
                        )
                    ).to(device)
                    if sa.removed_neurons
                    else None
                )
                if self.bf16:
                    linv_t = linv_t.to(torch.bfloat16)
                self.lsa_mode.append(("fused", keep, linv_t))
                wtrains.append(xw)
                woffs.append(woffs[-1] + xw.shape[0])
                consts[c] = const
                any_fused = True
            if any_fused:
                self.lsa_wtrainS = torch.cat(wtrains).contiguous()
                self.lsa_wnormS = (
                    self.lsa_wtrainS * self.lsa_wtrainS
                ).sum(dim=1).contiguous()
                if self.bf16:
                    self.lsa_wtrainS16 = self.lsa_wtrainS.to(
                        torch.bfloat16
                    ).contiguous()
                    f = self.lsa_wtrainS16.float()
                    self.lsa_wnormS16 = (f * f).sum(dim=1).contiguous()
                    del f
                self.lsa_nseg = torch.tensor(
                    woffs, dtype=torch.int32, device=device
                )
                self.lsa_jb_max = max(
                    1,
                    max(
                        (woffs[c + 1] - woffs[c] + 127) // 128
                        for c in range(self.num_classes)
                    ),
                )
                self.lsa_d = d_ref
                self.lsa_consts = torch.tensor(
                    consts, dtype=torch.float32, device=device
                )
                self.lsa_ready = True

        self.fast = (
            fast is not False
            and os.environ.get("TIP_NO_FAST_SCORING") != "1"
            and self._fast_eligible(lsa)
        )
        if self.fast:
            self._build_fast_tables()

    # ------------------------------------------------------------------
    # Sync-free path: device segment plan + gathered kernels. The batch is
    # never class-sorted or padded in memory; a plan kernel writes the
    # padded-row -> source-row map, the pairwise / whiten kernels gather
    # source rows through it and the combine kernels scatter the final
    # scores back, so a call is ~9 launches with no host<->device copy and
    # no host loop over classes (docs/kernels.md, "grouped scoring,
    # sync-free path").
    # ------------------------------------------------------------------

    def _fast_eligible(self, lsa) -> bool:
        if not self.bf16 or self.shard_train:
            return False
        if torch.device(self.device).type != "cuda":
            return False
        if self.trainS.shape[1] % 8 != 0:
            return False
        if self.num_classes > 256:
            return False
        if lsa is not None and any(m[0] == "fallback" for m in self.lsa_mode):
            return False
        if self.lsa_ready and self.lsa_d > self.ext.grouped_whiten_max_features():
            return False
        return True

    def _build_fast_tables(self):
        dev, c = self.device, self.num_classes
        self._ws = {}
        self._plan_event = None
        if not self.lsa_ready:
            return
        d = self.lsa_d
        keep = np.zeros((c, d), dtype=np.int32)
        # per-class matrices zero-padded to [pad16(d), pad32(d)]: aligned
        # 16-byte fragment loads, no tail handling in the kernel
        wt = torch.zeros(
            c, (d + 15) // 16 * 16, (d + 31) // 32 * 32,
            dtype=torch.bfloat16, device=dev,
        )
        fused = np.zeros(c, dtype=np.int32)
        const = self.lsa_consts.cpu().numpy().astype(np.float32).copy()
        for cls, mode in enumerate(self.lsa_mode):
            if mode[0] == "fused":
                _, kidx, linv_t = mode
                keep[cls] = (
                    kidx.cpu().numpy() if kidx is not None else np.arange(d)
                )
                # K-contiguous per output column: wt[c, n, k] = linv_t[k, n]
                wt[cls, :d, :d] = linv_t.t()
                fused[cls] = 1
            else:
                const[cls] = mode[1]
        self._keep_cols = int(keep.max()) + 1  # widest source column read
        self.lsa_keep = torch.from_numpy(keep).to(dev)
        self.lsa_wt = wt.contiguous()
        self.lsa_cls_fused = torch.from_numpy(fused).to(dev)
        self.lsa_cls_const = torch.from_numpy(const).to(dev)

    def _workspaces(self, b: int, d_at: int):
        """Per-(B, D) scratch, reused from call to call: each call ends with
        the main stream waiting on the LSA stream, so the next call's
        kernels are ordered after every reader. Nothing read into an output
        depends on what a previous call left here."""
        ws = self._ws.get((b, d_at))
        if ws is not None:
            return ws
        if len(self._ws) >= 4:
            self._ws.clear()
        dev, c = self.device, self.num_classes
        bp = self.ext.segment_plan_rows(b, c)
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        ws = {
            "tseg": torch.empty(c + 1, **i32),
            "rowmap": torch.empty(bp, **i32),
            "dest": torch.empty(b, **i32),
            "an": torch.empty(b, **f32),
            "pval": torch.empty(self.jb_max, bp, **f32),
            "pidx": torch.empty(self.jb_max, bp, **i32),
            "dist": torch.empty(b, **f32),
            "idx": torch.empty(b, **i32),
        }
        if self.lsa_ready:
            ws["white"] = torch.empty(
                bp, self.lsa_d, dtype=torch.bfloat16, device=dev
            )
            ws["wan"] = torch.empty(bp, **f32)
            ws["pkde"] = torch.empty(self.lsa_jb_max, bp, 2, **f32)
        self._ws[(b, d_at)] = ws
        return ws

    def _gaussian_launch(self, ats, pred, plan, main_stream):
        """Enqueue every Gaussian scorer on the Gaussian side stream, ordered
        after what the main stream holds now (the segment plan, on the fast
        path). Returns the [names, B] score tensor; the caller makes the main
        stream wait on the side stream before handing anything out, which is
        also what lets the next call reuse the scorers' workspaces.

        ``plan`` is the call's (tseg, rowmap) over the predicted classes or
        None. A by-class scorer whose groups are the classes reuses it; a
        kmeans-discriminated one (or one with other groups, or a batch over
        the workspace cap) plans from its own group ids."""
        from ..ops import hip_ops

        names = list(self.gaussian)
        x = ats if ats.dtype == torch.bfloat16 else ats.float()
        x = x.contiguous()
        out = torch.full(
            (len(names), ats.shape[0]), float("inf"),
            dtype=torch.float32, device=ats.device,
        )
        if not hasattr(self, "_gauss_stream"):
            self._gauss_stream = torch.cuda.Stream()
        ready = torch.cuda.Event()
        ready.record(main_stream)
        # x may be a temporary of the main stream's pool: keep its memory
        # from being handed out again before the side stream has read it
        x.record_stream(self._gauss_stream)
        with torch.cuda.stream(self._gauss_stream):
            self._gauss_stream.wait_event(ready)
            for k, name in enumerate(names):
                sa = self.gaussian[name]
                tables = sa.tables(ats.device)
                if (
                    plan is not None
                    and sa.by_class
                    and sa.identity_groups
                    and tables.G == self.num_classes
                    and ats.shape[0] <= tables.chunk_rows()
                ):
                    hip_ops.grouped_gaussian_into(
                        x, tables, plan[0], plan[1], out[k]
                    )
                else:
                    group = sa.groups_of(sa.mode_ids(x, pred))
                    hip_ops.grouped_gaussian_scores_tables(
                        x, group, tables, out=out[k]
                    )
        return out

    @torch.no_grad()
    def score_all(
        self, ats: torch.Tensor, pred: torch.Tensor
    ) -> Dict[str, torch.Tensor]:
        """Every served score of one batch: ``"dsa"``, ``"pc-lsa"`` (when an
        LSA was fitted) and one entry per ``gaussian`` scorer. ``"dsa"`` /
        ``"pc-lsa"`` are what ``__call__`` returns; a Gaussian entry equals
        ``fuse()(ats, pred)`` of its scorer. The Gaussian kernels stay exact
        fp32 in bf16 mode and overlap the DSA / LSA kernels on a side
        stream."""
        if not self.gaussian:
            dsa, lsa = self(ats, pred)
            gauss = None
        elif self.fast and ats.is_cuda:
            dsa, lsa, gauss = self._fast_call(ats, pred, with_gaussian=True)
        else:
            main_stream = torch.cuda.current_stream()
            gauss = self._gaussian_launch(ats, pred, None, main_stream)
            dsa, lsa = self(ats, pred)
            main_stream.wait_stream(self._gauss_stream)
        res = {"dsa": dsa}
        if lsa is not None:
            res["pc-lsa"] = lsa
        for k, name in enumerate(self.gaussian):
            res[name] = gauss[k]
        return res

    def _fast_call(self, ats, pred, with_gaussian: bool = False):
        b, d_at = ats.shape
        assert d_at == self.trainS16.shape[1], "AT width differs from the fit"
        ext, ws = self.ext, self._workspaces(b, d_at)
        a16 = ats.to(torch.bfloat16).contiguous()  # no-op for bf16 ATs
        pred = pred.to(torch.int64).contiguous()
        ext.segment_plan_out(
            pred, self.num_classes, ws["tseg"], ws["rowmap"], ws["dest"]
        )
        ext.rownorm_bf16_out(a16, ws["an"])
        # unplaced rows (prediction outside the fitted range) stay +inf
        out = torch.full(
            (2, b), float("inf"), dtype=torch.float32, device=ats.device
        )
        main_stream = torch.cuda.current_stream()
        gauss = None
        if with_gaussian:
            gauss = self._gaussian_launch(
                ats, pred, (ws["tseg"], ws["rowmap"]), main_stream
            )
        if self.lsa_ready:
            assert self._keep_cols <= d_at
            if not hasattr(self, "_lsa_stream"):
                self._lsa_stream = torch.cuda.Stream()
            if self._plan_event is None:
                self._plan_event = torch.cuda.Event()
            self._plan_event.record(main_stream)
            with torch.cuda.stream(self._lsa_stream):
                self._lsa_stream.wait_event(self._plan_event)
                ext.grouped_whiten_bf16(
                    a16, ws["rowmap"], ws["tseg"], self.lsa_nseg,
                    self.lsa_keep, self.lsa_wt, ws["white"],
                )
                ext.rownorm_bf16_out(ws["white"], ws["wan"], ws["tseg"])
                ext.grouped_kde_plan(
                    ws["white"], self.lsa_wtrainS16, ws["tseg"],
                    self.lsa_nseg, ws["rowmap"], ws["wan"],
                    self.lsa_wnormS16, self.lsa_cls_fused,
                    self.lsa_cls_const, self.lsa_jb_max, ws["pkde"], out[1],
                )
        ext.grouped_rowmin_plan(
            a16, self.trainS16, ws["tseg"], self.nseg, ws["rowmap"],
            ws["an"], self.bnormS16, self.btableS, self.jb_max,
            ws["pval"], ws["pidx"], out[0], ws["dist"], ws["idx"],
        )
        if self.lsa_ready:
            main_stream.wait_stream(self._lsa_stream)
        lsa_out = out[1] if self.lsa_ready else None
        if with_gaussian:
            main_stream.wait_stream(self._gauss_stream)
            return out[0], lsa_out, gauss
        return out[0], lsa_out

    def _lsa_lse(self, padded, bp, tseg_cpu, tseg):
        """Per-class whiten GEMMs + one grouped KDE launch (+ cross-rank
        logsumexp merge of the train-shard partials in shard mode).

        In bf16 mode `padded` is bf16, the whiten GEMM runs bf16 (hipBLASLt
        MFMA) and the KDE kernel consumes the bf16 coordinates directly."""
        wdtype = torch.bfloat16 if self.bf16 else torch.float32
        white = torch.zeros(bp, self.lsa_d, device=padded.device, dtype=wdtype)
        for c in range(self.num_classes):
            lo, hi = int(tseg_cpu[c]), int(tseg_cpu[c + 1])
            if hi <= lo or self.lsa_mode[c][0] != "fused":
                continue
            _, keep, linv_t = self.lsa_mode[c]
            seg = padded[lo:hi]
            if keep is not None:
                seg = seg.index_select(1, keep)
            white[lo:hi] = seg @ linv_t
        if self.bf16:
            w16 = white.contiguous()
            wf = w16.float()
            wan = (wf * wf).sum(dim=1).contiguous()
            lse = self.ext.grouped_kde_bf16(
                w16, self.lsa_wtrainS16, tseg, self.lsa_nseg, wan,
                self.lsa_wnormS16, self.lsa_jb_max,
            )
        else:
            lse = self.ext.grouped_kde(
                white.contiguous(), self.lsa_wtrainS, tseg, self.lsa_nseg,
                self.lsa_wnormS, self.lsa_jb_max,
            )
        if self.shard_train:
            from ..parallel.dist import gather_tensors

            lse = torch.logsumexp(torch.stack(gather_tensors(lse)), dim=0)
        return lse

    @staticmethod
    def _merge_rowmin(dist, idx):
        """Strict-less rank-ordered merge of (min, global argmin) partials —
        lowest rank holds the lowest global rows per class, so ties keep the
        single-device lowest-index rule."""
        from ..parallel.dist import gather_tensors
        from ..parallel.sharded import fold_rowmin_partials

        return fold_rowmin_partials(gather_tensors(dist), gather_tensors(idx))

    def _segment(self, ats: torch.Tensor, pred: torch.Tensor):
        """Class-sort + pad to 128-row segments."""
        counts = torch.bincount(pred, minlength=self.num_classes)
        counts_cpu = counts.cpu().numpy()  # the single step sync
        assert counts_cpu.shape[0] == self.num_classes, (
            "prediction outside the fitted class range"
        )
        padded = ((counts_cpu + 127) // 128) * 128
        tseg_cpu = np.zeros(self.num_classes + 1, dtype=np.int64)
        tseg_cpu[1:] = np.cumsum(padded)
        starts_cpu = np.zeros(self.num_classes, dtype=np.int64)
        starts_cpu[1:] = np.cumsum(counts_cpu)[:-1]
        order = torch.argsort(pred, stable=True)
        starts = torch.from_numpy(starts_cpu).to(pred.device)
        tseg_dev64 = torch.from_numpy(tseg_cpu).to(pred.device)
        sorted_pred = pred[order]
        intra = torch.arange(pred.shape[0], device=pred.device) - starts[sorted_pred]
        dest = tseg_dev64[sorted_pred] + intra
        return order, dest, tseg_cpu, tseg_dev64.to(torch.int32)

    @torch.no_grad()
    def __call__(
        self, ats: torch.Tensor, pred: torch.Tensor
    ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(dsa scores, lsa scores or None) for fp32 ATs [B, D] on device."""
        if self.fast and ats.is_cuda:
            return self._fast_call(ats, pred)
        b = ats.shape[0]
        order, dest, tseg_cpu, tseg = self._segment(ats, pred)
        bp = int(tseg_cpu[-1])
        pdtype = torch.bfloat16 if self.bf16 else torch.float32
        padded = torch.zeros(bp, ats.shape[1], device=ats.device, dtype=pdtype)
        padded[dest] = ats[order].to(pdtype)

        # DSA (main stream) and LSA whiten+KDE (side stream) are independent
        # given `padded`; overlap them.
        lse = None
        main_stream = torch.cuda.current_stream() if ats.is_cuda else None
        if self.lsa_ready and ats.is_cuda:
            if not hasattr(self, "_lsa_stream"):
                self._lsa_stream = torch.cuda.Stream()
            ready = torch.cuda.Event()
            ready.record(main_stream)
            with torch.cuda.stream(self._lsa_stream):
                self._lsa_stream.wait_event(ready)
                lse = self._lsa_lse(padded, bp, tseg_cpu, tseg)
                lse.record_stream(main_stream)

        if self.bf16:
            pf = padded.float()
            an = (pf * pf).sum(dim=1).contiguous()
            del pf
            dist, idx = self.ext.grouped_rowmin_bf16(
                padded.contiguous(), self.trainS16, tseg, self.nseg, an,
                self.bnormS16, self.jb_max,
            )
        else:
            dist, idx = self.ext.grouped_rowmin(
                padded.contiguous(), self.trainS, tseg, self.nseg,
                self.bnormS, self.jb_max,
            )
        if self.shard_train:
            idx = torch.where(
                idx >= 0, self.local2global[idx.clamp_min(0)], idx
            )
            dist, idx = self._merge_rowmin(dist, idx)
        dsa_sorted = torch.where(
            idx >= 0,
            dist / self.btableS[idx.clamp_min(0)],
            torch.full_like(dist, float("inf")),
        )
        dsa = torch.empty(b, device=ats.device)
        dsa[order] = dsa_sorted[dest]

        lsa = None
        if self.lsa_ready:
            if lse is None:  # CPU path (no side stream)
                lse = self._lsa_lse(padded, bp, tseg_cpu, tseg)
            else:
                main_stream.wait_stream(self._lsa_stream)
            cls_of_row = torch.bucketize(
                torch.arange(bp, device=ats.device), tseg.long()[1:], right=True
            )
            lsa_sorted = -(lse + self.lsa_consts[cls_of_row])
            # patch degraded / fallback classes
            for c in range(self.num_classes):
                mode = self.lsa_mode[c]
                if mode[0] == "fused":
                    continue
                lo, hi = int(tseg_cpu[c]), int(tseg_cpu[c + 1])
                if hi <= lo:
                    continue
                if mode[0] == "const":
                    lsa_sorted[lo:hi] = mode[1]
                else:  # fallback: per-class SA on the real rows
                    lsa_sorted[lo:hi] = mode[1](padded[lo:hi]).float().to(
                        ats.device
                    )
            lsa = torch.empty(b, device=ats.device)
            lsa[order] = lsa_sorted[dest]
        return dsa, lsa
