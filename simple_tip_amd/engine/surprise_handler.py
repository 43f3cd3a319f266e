"""Surprise-adequacy orchestration per model.

Capability parity with reference src/dnn_test_prio/handler_surprise.py:19-117
(same TESTED_SA configs, timing taxonomy [setup, pred, quant, cam], dynamic
surprise-coverage upper bound, per-dataset CAM). Train/test ATs stay resident
on device; SA hot loops route through the MFMA pairwise kernel via ops.
"""

import logging
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from ..config import NUM_SC_BUCKETS
from ..core.prioritizers import cam, cam_many
from ..core.surprise import (
    DSA,
    LSA,
    MDSA,
    MLSA,
    MultiModalSA,
    SurpriseCoverageMapper,
    resolve_kmeans_mode,
)
from ..core.timer import DeviceTimer
from .model_handler import BaseModel

logger = logging.getLogger(__name__)


class SurpriseHandler:
    """Fits on train ATs once, evaluates all SA variants on test sets."""

    TESTED_SA = {
        "dsa": lambda x, y: DSA(x, y, subsampling=0.3),
        "pc-lsa": lambda x, y: MultiModalSA.build_by_class(x, y, lambda a, p: LSA(a)),
        "pc-mdsa": lambda x, y: MultiModalSA.build_by_class(x, y, lambda a, p: MDSA(a)),
        "pc-mlsa": lambda x, y: MultiModalSA.build_by_class(
            x, y, lambda a, p: MLSA(a, num_components=3)
        ),
        "pc-mmdsa": lambda x, y, **kw: MultiModalSA.build_with_kmeans(
            x, y, lambda a, p: MDSA(a), potential_k=range(2, 6), subsampling=0.3, **kw
        ),
    }

    #: the Gaussian configurations MultiModalSA.fuse() applies to
    FUSABLE_SA = ("pc-mdsa", "pc-mlsa", "pc-mmdsa")

    def __init__(
        self,
        model,
        sa_layers: List[int],
        training_dataset,
        device=None,
        predict_batch: int = 512,
        dist_shard: bool = False,
        modal_sa_mode: str = "per_mode",
        cam_mode: str = "per_metric",
        kmeans_mode: str = "looped",
    ):
        from ..parallel.dist import get_world_size

        # "batched": pc-mmdsa's k-means discovery runs every restart of every
        # k in lockstep and scores all k from one pass over the distances
        # (core.kmeans.kmeans_fit_many / silhouette_scores_many); "looped"
        # (the default) fits one k after the other. TIP_KMEANS_MODE overrides.
        self.kmeans_mode = resolve_kmeans_mode(kmeans_mode)

        # "fused": the three Gaussian configurations (pc-mdsa, pc-mlsa,
        # pc-mmdsa) are fit as usual and then MultiModalSA.fuse()d, so every
        # evaluation scores all modes in one grouped launch. "per_mode" (the
        # default) keeps the per-mode loop. TIP_MODAL_SA_MODE overrides.
        modal_sa_mode = os.environ.get("TIP_MODAL_SA_MODE", modal_sa_mode)
        if modal_sa_mode not in ("per_mode", "fused"):
            raise ValueError(
                f"modal_sa_mode must be 'per_mode' or 'fused', got {modal_sa_mode!r}"
            )
        self.modal_sa_mode = modal_sa_mode
        # "batched": the surprise-coverage profiles of every (SA, dataset)
        # pair are ordered by one cam_many call (on the GPU one persistent
        # launch, a team of blocks per pair) instead of one cam call each
        # ("per_metric", the default); the orders are identical. Every
        # pair's cam time slot is then charged the WHOLE call, the rule of
        # CoverageWorker's fused modes. TIP_CAM_MODE overrides.
        cam_mode = os.environ.get("TIP_CAM_MODE", cam_mode)
        if cam_mode not in ("per_metric", "batched"):
            raise ValueError(
                f"cam_mode must be 'per_metric' or 'batched', got {cam_mode!r}"
            )
        self.cam_mode = cam_mode
        self.sa_layers = list(sa_layers)
        # dist_shard: shard AT-extraction and SA scoring over the test-input
        # axis across ranks (DP per SURVEY §2.4); train ATs are extracted
        # sharded then all-gathered so every rank fits identical SAs.
        self.dist_shard = bool(dist_shard) and get_world_size() > 1
        self.base_model = BaseModel(
            model,
            self.sa_layers,
            include_last_layer=True,
            device=device,
            predict_batch=predict_batch,
        )
        self.train_at_timer = DeviceTimer()
        with self.train_at_timer:
            if self.dist_shard:
                from ..parallel.dist import allgather_rows, shard_slice

                n = training_dataset.shape[0]
                ats_l, pred_l = self._acti_and_pred(
                    training_dataset[shard_slice(n)]
                )
                self.train_ats = allgather_rows(ats_l, n)
                self.train_pred = allgather_rows(pred_l, n)
            else:
                self.train_ats, self.train_pred = self._acti_and_pred(
                    training_dataset
                )

    def _acti_and_pred(self, dataset):
        """ATs and argmax predictions in one fused forward pass (K15)."""
        outputs = self.base_model.get_activations(dataset)
        assert len(outputs) == len(self.sa_layers) + 1
        ats = [o.reshape(o.shape[0], -1) for o in outputs[:-1]]
        flat = torch.cat(ats, dim=1) if len(ats) > 1 else ats[0]
        return flat, outputs[-1].argmax(dim=1)

    def evaluate_all(
        self, datasets: Dict[str, object], dsa_badge_size: Optional[int] = None
    ):
        """{sa_name: {ds_name: (scores, cam_order, [setup,pred,quant,cam])}}"""
        res = {}
        test_apt = {}
        for ds_name, dataset in datasets.items():
            t = DeviceTimer()
            with t:
                if self.dist_shard:
                    from ..parallel.dist import shard_slice

                    n = dataset.shape[0]
                    test_ats, test_pred = self._acti_and_pred(
                        dataset[shard_slice(n)]
                    )
                else:
                    n = None
                    test_ats, test_pred = self._acti_and_pred(dataset)
            test_apt[ds_name] = (test_ats, test_pred, t.get(), n)

        for sa_name, sa_func in self.TESTED_SA.items():
            res[sa_name] = {}
            setup_timer = DeviceTimer()
            with setup_timer:
                logger.info("Creating %s instance", sa_name)
                if sa_name == "pc-mmdsa" and self.kmeans_mode != "looped":
                    sa = sa_func(
                        self.train_ats, self.train_pred, kmeans_mode=self.kmeans_mode
                    )
                else:
                    sa = sa_func(self.train_ats, self.train_pred)
                if isinstance(sa, DSA) and dsa_badge_size is not None:
                    sa.badge_size = dsa_badge_size
                if self.modal_sa_mode == "fused" and sa_name in self.FUSABLE_SA:
                    sa = sa.fuse(device=self.train_ats.device)
            setup_time = self.train_at_timer.get() + setup_timer.get()

            for ds_name, (test_ats, test_pred, pred_time, n) in test_apt.items():
                sa_timer = DeviceTimer()
                with sa_timer:
                    logger.info("Calculating %s for %s", sa_name, ds_name)
                    sa_vals = sa(test_ats, test_pred)
                    if self.dist_shard:
                        # publish the per-input score shard (tiny all-gather)
                        from ..parallel.dist import allgather_rows

                        sa_vals = allgather_rows(sa_vals.contiguous(), n)
                res[sa_name][ds_name] = (sa_vals, [setup_time, pred_time, sa_timer.get()])

        if self.cam_mode == "batched":
            return self._cam_batched(res, datasets)
        for sa_name in self.TESTED_SA.keys():
            for ds_name in datasets.keys():
                sa_vals, times = res[sa_name][ds_name]
                cam_timer = DeviceTimer()
                with cam_timer:
                    vals_t, profiles = self._coverage_profile(sa_vals)
                    cam_order = np.array(list(cam(vals_t.float(), profiles)))
                times = times + [cam_timer.get()]
                sa_np = vals_t.double().cpu().numpy()
                res[sa_name][ds_name] = (sa_np, cam_order, times)
        return res

    @staticmethod
    def _coverage_profile(sa_vals):
        """(values as a tensor, their surprise-coverage profile) with the
        dynamic upper bound: the largest finite value."""
        vals_t = torch.as_tensor(sa_vals)
        finite = vals_t[torch.isfinite(vals_t)]
        upper = float(finite.max()) if finite.numel() else 1.0
        mapper = SurpriseCoverageMapper(NUM_SC_BUCKETS, upper)
        return vals_t, mapper.get_coverage_profile(vals_t)

    def _cam_batched(self, res, datasets):
        """The final loop of ``evaluate_all`` with every (SA, dataset) pair
        ordered by one ``cam_many`` call."""
        keys = [(sa, ds) for sa in self.TESTED_SA.keys() for ds in datasets.keys()]
        cam_timer = DeviceTimer()
        with cam_timer:
            pairs = [self._coverage_profile(res[sa][ds][0]) for sa, ds in keys]
            orders = cam_many(
                [v.float() for v, _ in pairs], [p for _, p in pairs]
            )
        for (sa, ds), (vals_t, _), order in zip(keys, pairs, orders):
            times = res[sa][ds][1] + [cam_timer.get()]  # the whole call, each
            sa_np = vals_t.double().cpu().numpy()
            res[sa][ds] = (sa_np, np.array(order), times)
        return res
