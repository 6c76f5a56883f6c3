"""``evaluation()`` on this target: the reference's loop (src/tools/evaluation.py:36-100) -- same running
averages, same score/error records (ESA score via SPEUtils.get_score, std and median absolute deviation of the
per-image errors) -- driving any object with ``predict(images) -> (pose, latency_ms)`` (SPEMi355x).

Keypoint mode with MODEL.HEAD.KEYPOINTS_REFINE_ITERS > 0 (``SPEMi355x(..., keypoint_refine=config.keypoint_refine(cfg))``)
scores the pose refined behind EPnP in both loops: ``predict`` returns it, and ``eval_pipeline`` configures every slot
of the device loop's ``StreamPipeline`` with it. MODEL.HEAD.KEYPOINTS_CONSENSUS_PX > 0
(``keypoint_consensus=config.keypoint_consensus(cfg)``) puts the 3-point consensus in front of that refinement in the same
way: the scored pose is the one refined on the inliers."""
from __future__ import annotations

from typing import Any, Dict, Iterable, Tuple

import numpy as np


def mad(data) -> float:
    """Median absolute deviation (evaluation.py:17-33)."""
    med = np.median(data)
    return float(np.median(np.abs(np.asarray(data) - med)))


class RunningAverage:
    """Batch-size weighted running means (src/tools/utils.py:16-60)."""

    def __init__(self, keys):
        self.tot = {k: 0.0 for k in keys}
        self.n = {k: 0 for k in keys}

    def update(self, values: Dict[str, float], batch_size: int = 1) -> None:
        for k, v in values.items():
            self.tot[k] += float(v) * batch_size
            self.n[k] += batch_size

    def get(self, k: str) -> float:
        return self.tot[k] / self.n[k] if self.n[k] else 0.0


def evaluation(spe_model: Any, dataloader: Dict[str, Iterable], spe_utils,
               split: Tuple[str, ...] = ('test', 'valid')):
    rec_score = {x: {'ori': [], 'pos': [], 'esa': []} for x in split}
    rec_error = {x: {'ori': [], 'pos': [], 'ori_std': [], 'pos_std': [], 'ori_mad': [], 'pos_mad': []} for x in split}
    for phase in split:
        error = {'ori': [], 'pos': []}
        running = RunningAverage(('esa_score', 'ori_score', 'pos_score', 'ori_error', 'pos_error'))
        for images, targets in dataloader[phase]:
            pose, _ = spe_model.predict(images['torch'])
            targets = {k: v.detach().cpu().numpy() for k, v in targets.items()}
            running.update(spe_utils.get_score(targets, pose), images['torch'].size(0))
            error['pos'].extend(np.linalg.norm(targets['pos'] - pose['pos'], axis=1))
            s = np.abs(np.sum(pose['ori'] * targets['ori'], axis=1, keepdims=True))
            s[s > 1] = 1
            error['ori'].extend((2 * np.arccos(s) * 180 / np.pi).reshape(-1))
        rec_score[phase]['ori'].append(running.get('ori_score'))
        rec_score[phase]['pos'].append(running.get('pos_score'))
        rec_score[phase]['esa'].append(running.get('esa_score'))
        rec_error[phase]['ori'].append(running.get('ori_error'))
        rec_error[phase]['pos'].append(running.get('pos_error'))
        rec_error[phase]['ori_std'].append(float(np.std(error['ori'])))
        rec_error[phase]['pos_std'].append(float(np.std(error['pos'])))
        rec_error[phase]['ori_mad'].append(mad(error['ori']))
        rec_error[phase]['pos_mad'].append(mad(error['pos']))
    return rec_score, rec_error


def evaluation_device(spe_model: Any, dataloader: Dict[str, Iterable], spe_utils,
                      split: Tuple[str, ...] = ('test', 'valid'), capacity: int = 0):
    """``evaluation()`` with the scoring on the device: the batches go through a depth-3 ``StreamPipeline`` of the
    model's weights (``SPEMi355x.eval_pipeline``), each followed on its stream by a scoring step against its targets
    (``PoseScorer``, csrc/k_score.hip); nothing is copied back and nothing synchronises per batch. One ``result()``
    per phase yields the same records. The means are those of all images (``evaluation()`` weights its per-batch means
    by the batch size: the same number up to rounding); std and MAD are taken over the float32 per-image errors.

    Raises the reference's ValueError (spe_utils.py:137) at the end of a phase if a row's |q . q_true| exceeded 1.01,
    and the decode's ValueError if a row's decode status was nonzero. ``capacity``: rows per phase (default: the
    phase's dataset size when the loader tells it, else 2^20)."""
    from ..score import FLAG_DOT, FLAG_STATUS
    rec_score = {x: {'ori': [], 'pos': [], 'esa': []} for x in split}
    rec_error = {x: {'ori': [], 'pos': [], 'ori_std': [], 'pos_std': [], 'ori_mad': [], 'pos_mad': []} for x in split}
    pipe = spe_model.eval_pipeline(3)
    dev = spe_model.device
    for phase in split:
        loader = dataloader[phase]
        cap = capacity
        if cap <= 0:
            ds = getattr(loader, 'dataset', None)
            cap = len(ds) if ds is not None and hasattr(ds, '__len__') else (1 << 20)
        scorer = pipe.engine.scorer(1, 1, max(1, min(cap, 1 << 20)))
        try:
            for images, targets in loader:
                x = images['torch'].to(dev, non_blocking=True).contiguous()
                if spe_model.keypoint_mode:
                    pipe.submit_keypoints(x, score=(scorer, targets))
                else:
                    pipe.submit(x, spe_model.ori_mode, spe_model.pos_mode, want_soft=False, score=(scorer, targets))
            res = {k: float(v[0, 0]) for k, v in scorer.result().items()}
        finally:
            scorer.close()
        flags = int(res['flags'])
        if flags & FLAG_DOT:
            raise ValueError('Intermediate sum issue due to error in model prediction (orientation)')
        if flags & FLAG_STATUS:
            raise ValueError('Error during pose decoding (a row of the phase has a nonzero decode status)')
        if res['n_dropped']:
            raise ValueError(f'{int(res["n_dropped"])} images of phase {phase!r} exceeded the scorer capacity {cap}')
        rec_score[phase]['ori'].append(res['ori_score'])
        rec_score[phase]['pos'].append(res['pos_score'])
        rec_score[phase]['esa'].append(res['esa_score'])
        for k in ('ori', 'pos'):
            rec_error[phase][k].append(res[f'{k}_error'])
            rec_error[phase][f'{k}_std'].append(res[f'{k}_std'])
            rec_error[phase][f'{k}_mad'].append(res[f'{k}_mad'])
    return rec_score, rec_error
