"""Batch-level pipelining of the hot path over HIP streams.

The backbone's late blocks run one workgroup per CU at low occupancy and the head/decode kernels are small, so
a single stream leaves the GPU partly idle at the end of every batch. ``StreamPipeline`` keeps up to ``depth``
batches in flight, batch k on stream k % depth with its own SPEF context (workspace), so batch k's tail kernels
overlap batch k+1's front kernels. Weights are loaded into every context from the same blob (13.5 MB each for
the fp16 URSONet model -- nothing next to 288 GB of HBM).

This is the serving-side counterpart of the reference's evaluation loop (``tools/evaluation.py:63-90``), which
runs ``SPETorch.predict`` batch after batch; each submitted batch is still the complete forward + decode.

``use_graphs()`` (optional) records each (stream, input batch) pair's forward + decode once as a HIP graph and
replays it on later submits of the same input tensor: one graph launch per batch instead of ~20 kernel launches.
Its decode outputs then live in the graph's memory and are overwritten when that pair is submitted again. A recorded
graph holds fixed device addresses (the engine's workspace, the stream's output buffers, the decode tables), so its
key carries the engine's ``epoch`` (bumped by every workspace reallocation and state change) and the output buffers'
addresses, and a stream's graphs are dropped as soon as either moves.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from .engine import Engine


class StreamPipeline:
    def __init__(self, blob, device, depth: int = 3, ori_bins: Optional[np.ndarray] = None,
                 pos_grid: Optional[np.ndarray] = None, comm=None, root: int = 0):
        """``blob``: the packed weights (host bytes or device tensor). With ``comm`` (a ``shard.RcclComm``), only
        rank ``root`` passes a blob (the others None) and every context receives the root's weights over RCCL
        (``spef_bcast_weights``, collective)."""
        assert depth >= 1
        self.device = torch.device(device)
        self.depth = depth
        self.engines: List[Engine] = [Engine(blob, self.device) for _ in range(depth)]
        if comm is not None:
            for e in self.engines:
                e.bcast_weights(comm, root)
        for e in self.engines:
            e.set_decode_tables(ori_bins, pos_grid)
        self.streams = [torch.cuda.Stream(self.device) for _ in range(depth)]
        self._bufs = [None] * depth
        self._next = 0
        self.graphs = False
        self._graphs = {}

    def use_graphs(self, on: bool = True) -> None:
        self.graphs = bool(on)
        if not on:
            self._graphs.clear()

    @property
    def engine(self) -> Engine:
        return self.engines[0]

    def reserve(self, B: int, H: int, W: int) -> None:
        for e in self.engines:
            e.reserve(B, H, W)

    def submit(self, frames: torch.Tensor, ori_mode: int = L.CLASSIFICATION, pos_mode: int = L.REGRESSION,
               want_soft: bool = True, video=None, score=None, track=None, want_cov: bool = False,
               floor_var=(0.0, 0.0)) -> dict:
        """Enqueue forward + decode of one batch on the next stream; returns the decode dict (device tensors,
        valid once that stream reaches them -- ``synchronize()`` or the dict's 'event').

        ``video``: a ``VideoFilter`` (``Engine.video_filter``) whose streams this batch holds, time-major (T *
        n_streams frames, classification heads, ``want_soft``). Its step is enqueued on the slot's stream after the
        decode -- outside the slot's recorded graph -- and ordered after the previous submit's step by an event:
        the forwards of the slots still overlap, only the filter steps serialise. The filtered result is the
        dict's 'video' entry (``VideoFilter.step``), and 'event' then covers it too.

        ``score``: ``(scorer, targets)`` -- a ``PoseScorer`` (``Engine.scorer``) whose groups this batch holds,
        time-major, and the batch's true poses ({'ori', 'pos'}; device tensors, or host arrays that are copied).
        The scoring step is enqueued on the slot's stream after the decode (and after the video step: track 0 then
        logs the still poses, track 1 the filtered ones), outside the recorded graph, and ordered after the previous
        submit's scoring step by an event exactly as the video steps are.

        ``track``: a ``PoseTracker`` (``Engine.tracker``) whose streams this batch holds, time-major; any head. Its
        step is enqueued on the slot's stream after the decode, outside the recorded graph, and ordered after the
        previous submit's step through ``track.last_event`` exactly as ``video=`` is. The result is the dict's
        'track' entry (``PoseTracker.step``); with ``score`` as well, track 1 logs the tracked poses (flagged only
        where a row passed through without a track).

        ``want_cov`` (off by default): ``Engine.decode_cov`` is enqueued on the slot's stream after the decode, outside
        the recorded graph like the tracker step, and adds 'cov' / 'cov_status' to the dict -- so ``track=`` picks the
        PDFs' own covariance up as the measurement covariance. A regression head gets the tracker's ``r`` (without a
        tracker: ``spe.track.DEFAULTS['r']``); ``floor_var`` is added to a classification head's diagonal. Needs
        ``want_soft``."""
        i = self._next
        self._next = (i + 1) % self.depth
        eng, s = self.engines[i], self.streams[i]
        B = frames.shape[0]
        buf = self._bufs[i]
        if buf is None or buf[0].shape[0] != B:
            buf = (torch.empty((B, eng.n_out0), dtype=torch.float32, device=self.device),
                   torch.empty((B, eng.n_out1), dtype=torch.float32, device=self.device) if eng.n_out1 else None)
            self._bufs[i] = buf
            self._drop_graphs(i)                                 # recorded against the previous buffers
        s.wait_stream(torch.cuda.current_stream(self.device))   # frames were produced on the caller's stream
        if video is not None:
            assert ori_mode == L.CLASSIFICATION and pos_mode == L.CLASSIFICATION and want_soft, \
                'the video filter needs both soft PDFs'
            assert B % video.n_streams == 0, f'{B} frames are not whole time steps of {video.n_streams} streams'
        if self.graphs:
            dec = self._submit_graph(i, eng, s, buf, frames, ori_mode, pos_mode, want_soft)
        else:
            with torch.cuda.stream(s):
                frames.record_stream(s)
                raw0, raw1 = eng.forward(frames, *buf)
                dec = eng.decode(ori_mode, pos_mode, raw0, raw1, want_soft=want_soft)
                ev = torch.cuda.Event()
                ev.record(s)
            dec['raw0'], dec['raw1'] = raw0, raw1
            dec['event'] = ev
        if want_cov:
            assert want_soft, 'the covariance is computed from the soft PDFs'
            from .spe.track import DEFAULTS
            with torch.cuda.stream(s):
                eng.decode_cov(dec, ori_mode, pos_mode, fixed_var=track.params['r'] if track is not None else
                               DEFAULTS['r'], floor_var=floor_var)
                ev = torch.cuda.Event()
                ev.record(s)
            dec['event'] = ev
        if video is not None:
            with torch.cuda.stream(s):
                if video.last_event is not None:
                    s.wait_event(video.last_event)       # the filter's state: steps in submit order
                dec['video'] = video.step(dec, B // video.n_streams, engine=eng)
                ev = torch.cuda.Event()
                ev.record(s)
            video.last_event = dec['event'] = ev
        if track is not None:
            assert video is None, 'one batch goes through the video filter or the tracker, not both'
            self._track(s, dec, track, eng)
        if score is not None:
            self._score(s, dec, score, dec.get('video') or self._tracked_for_score(s, dec))
        return dec

    def _track(self, s, dec: dict, track, eng) -> None:
        B = dec['ori'].shape[0]
        assert B % track.n_streams == 0, f'{B} frames are not whole time steps of {track.n_streams} streams'
        with torch.cuda.stream(s):
            if track.last_event is not None:
                s.wait_event(track.last_event)           # the tracker's state: steps in submit order
            dec['track'] = track.step(dec, B // track.n_streams, engine=eng)
            ev = torch.cuda.Event()
            ev.record(s)
        track.last_event = dec['event'] = ev

    @staticmethod
    def _tracked_for_score(s, dec: dict):
        """The tracked poses as the scorer takes them: a row counts as failed only where it passed through."""
        if 'track' not in dec:
            return None
        with torch.cuda.stream(s):
            return dict(dec['track'], status=dec['track']['track_status'] & 8)

    def _score(self, s, dec: dict, score, video_dec=None) -> None:
        scorer, targets = score
        B = dec['ori'].shape[0]
        assert B % scorer.n_groups == 0, f'{B} rows are not whole time steps of {scorer.n_groups} groups'
        with torch.cuda.stream(s):
            tg = scorer.targets(targets)                 # host targets: copied before the wait below
            if scorer.last_event is not None:
                s.wait_event(scorer.last_event)          # the logs' counts: steps in submit order
            scorer.step(0, dec, tg, B // scorer.n_groups)
            if video_dec is not None:
                scorer.step(1, video_dec, tg, B // scorer.n_groups)
            ev = torch.cuda.Event()
            ev.record(s)
        scorer.last_event = dec['event'] = ev

    def _drop_graphs(self, i: int) -> None:
        for k in [k for k in self._graphs if k[0] == i]:
            del self._graphs[k]

    def _submit_graph(self, i, eng, s, buf, frames, ori_mode, pos_mode, want_soft) -> dict:
        _, B, H, W = eng._layout(frames)
        eng.reserve(B, H, W)                                     # any reallocation happens before the key is taken
        bufkey = tuple(0 if t is None else t.data_ptr() for t in buf)
        key = (i, frames.data_ptr(), tuple(frames.shape), frames.dtype, ori_mode, pos_mode, want_soft, eng.epoch,
               bufkey)
        stale = [k for k in self._graphs if k[0] == i and (k[7] != eng.epoch or k[8] != bufkey)]
        for k in stale:                                          # their workspace / buffers may be freed memory now
            del self._graphs[k]
        ent = self._graphs.get(key)
        if ent is None:
            with torch.cuda.stream(s):   # one eager pass first: lazily set kernel attributes stay out of the capture
                raw0, raw1 = eng.forward(frames, *buf)
                eng.decode(ori_mode, pos_mode, raw0, raw1, want_soft=want_soft)
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                raw0, raw1 = eng.forward(frames, *buf)
                dec = eng.decode(ori_mode, pos_mode, raw0, raw1, want_soft=want_soft)
            ent = self._graphs[key] = (g, dec)
        g, dec0 = ent
        with torch.cuda.stream(s):
            frames.record_stream(s)
            g.replay()
            ev = torch.cuda.Event()
            ev.record(s)
        dec = dict(dec0)
        dec['raw0'], dec['raw1'] = buf
        dec['event'] = ev
        return dec

    def set_keypoints(self, kp3d: np.ndarray, K: np.ndarray, nu: float, nv: float, dist=None) -> None:
        for e in self.engines:
            e.set_keypoints(kp3d, K, nu, nv, dist)

    def set_keypoint_refine(self, max_iters=None, huber_px: float = 0.0) -> None:
        """``Engine.set_keypoint_refine`` on every slot: ``submit_keypoints`` (and the scorer behind it) then use the
        pose refined behind EPnP. ``max_iters`` 0 or None turns it off."""
        for e in self.engines:
            e.set_keypoint_refine(max_iters, huber_px)

    def set_keypoint_consensus(self, inlier_px=None, min_inliers=None) -> None:
        """``Engine.set_keypoint_consensus`` on every slot: ``submit_keypoints`` then runs the 3-point consensus
        between EPnP and the refinement. ``inlier_px`` 0 or None turns it off."""
        for e in self.engines:
            e.set_keypoint_consensus(inlier_px, min_inliers)

    def submit_keypoints(self, frames: torch.Tensor, score=None, track=None) -> dict:
        """Keypoint mode: forward (KeypointRegressionHead) + sigmoid + batched EPnP (+ the pose refinement, when
        ``set_keypoint_refine`` turned it on) of one batch on the next stream; returns the decode dict of
        Engine.decode_keypoints plus 'raw' and 'event' (as submit()). ``score``, ``track``: as in ``submit``; with
        the refinement on, the tracker gets the refined pose's covariance (the dict then has 'cov')."""
        i = self._next
        self._next = (i + 1) % self.depth
        eng, s = self.engines[i], self.streams[i]
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            frames.record_stream(s)
            raw, _ = eng.forward(frames)   # allocated on s: every returned tensor belongs to this batch alone
            dec = eng.decode_keypoints(raw, want_cov=track is not None)
            ev = torch.cuda.Event()
            ev.record(s)
        dec['raw'] = raw
        dec['event'] = ev
        if track is not None:
            self._track(s, dec, track, eng)
        if score is not None:
            scored = dec
            if 'ori_epnp' in dec:   # the refinement's bits 16 / 32 are informational, not decode failures
                with torch.cuda.stream(s):
                    scored = dict(dec, status=dec['status'] & 15)
            self._score(s, scored, score, self._tracked_for_score(s, dec))
            dec['event'] = scored['event']
        return dec

    def synchronize(self) -> None:
        for s in self.streams:
            s.synchronize()

    def close(self) -> None:
        self.synchronize()
        self._graphs.clear()
        for e in self.engines:
            e.close()
        self.engines = []
