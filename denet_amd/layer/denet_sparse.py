"""`DNS` — DeNet sparse sampling layer. Mirrors denet/layer/denet_sparse.py (DeNetSparseLayer :26-218):
get_samples (:117-145) = corner detector -> build_samples; get_target (:164-206) = training-time RoI list
editing with the stdlib `random` module (random trim, random boxes, ground-truth injection) -> set_samples
(:155-161); the graph node is the sparse RoI gather (DeNetSparseOp, denet_sparse_op.py).

Differences by construction: the corner map never leaves the device — build_samples runs as HIP kernels
(csrc/samples.hip) and only the <= sample_count boxes per image come back for the Python-side editing; the
backbone is not run a second time (the reference compiles a separate `corner_func`). The RoI lists are kept as
float64 arrays (the values of the reference's Python floats); `sample_bbox_list` materialises the reference's
list-of-tuples view on demand."""
import math
import os
import random

import numpy

from . import AbstractLayer, Act, get_train
from .. import common
from ..common import logging
from .. import ops

TAP_THEANO = 0   # denet_sparse.py:72-84 (Theano CPU path, canonical per north star)
TAP_CUDA = 1     # denet_sparse_op.py:65-71
TAP_BILINEAR = 2  # opt-in, no reference counterpart (csrc/sparse_bilinear.hip): rule 0's coordinate, not rounded
TAP_RULES = (TAP_THEANO, TAP_CUDA, TAP_BILINEAR)


from .roi_handoff import (PyRandomMirror, py_random_doubles, RoiHandoff)      # noqa: F401 (re-exported)
from . import roi_handoff as _RH


class DeNetSparseLayer(RoiHandoff, AbstractLayer):
    type_name = "denet-sparse"
    # coverage statistics are log output only in the reference (denet_sparse.py:172-182); off by default because
    # the O(GT x RoI) Python loop is pure host overhead
    log_coverage = False

    def __init__(self, layers, grid_size=3, sample_num=16, corner_threshold=0.01, random_sample=0.0, local_max=0,
                 nms_threshold=0.7, sample_gt=True, version="v2", json_param={}, tap_rule=TAP_THEANO):
        super().__init__(layer_index=len(layers))
        self.input = layers[-1].output
        self.input_shape = layers[-1].output_shape
        self.batch_size = self.input_shape[0]

        self.grid_size = json_param.get("gridSize", grid_size)
        self.sample_num = json_param.get("sampleNum", sample_num)
        self.sample_gt = json_param.get("sampleGT", sample_gt)
        self.corner_threshold = json_param.get("cornerThreshold", corner_threshold)
        self.nms_threshold = json_param.get("nmsThreshold", nms_threshold)
        self.random_sample = json_param.get("randomSample", random_sample)
        self.local_max = json_param.get("localMax", local_max)
        self.version = json_param.get("version", version)
        self.tap_rule = json_param.get("tapRule", tap_rule)
        if isinstance(self.tap_rule, bool) or self.tap_rule not in TAP_RULES:
            raise ValueError("denet-sparse: tapRule must be 0 (theano), 1 (cuda) or 2 (bilinear), got %r" % (self.tap_rule,))
        self.tap_rule = int(self.tap_rule)

        self.corner_max = 1024
        self.thread_num = self.batch_size
        self.sample_count = self.sample_num * self.sample_num

        self.corner_layer = common.find_layers(layers, "denet-corner", True)
        assert self.corner_layer is not None, "denet-corner layer required before spare layer!"
        # nms_threshold < 1 turns on apply_cluster (denet_sparse.cc:541-542): the device proposal then returns the
        # 10 * sn^2 best candidates (the clustering input, :171-175) instead of sn^2 and the grouping runs on the host - or,
        # opt-in (ops.CLUSTER_DEVICE), on the device (csrc/cluster.hip), which hands an sn^2 list on like a layer without clustering
        self.cluster = self.nms_threshold < 1.0
        self.proposal_count = 10 * self.sample_num * self.sample_num if self.cluster else self.sample_num * self.sample_num

        self.sample_pr = []        # per image float64 [n]      (the three host-side views may be PENDING: _resolve_edit)
        self.sample_boxes = []     # per image float64 [n,4]
        self.sample_bbox_f32 = None
        self.sample_bbox = None    # device [B*sn*sn, 4]
        self.output_feat = self.grid_size * self.grid_size * self.corner_layer.sample_shape[1] + 2
        self.output_shape = (self.batch_size, self.output_feat, self.sample_num, self.sample_num)
        self.output = Act(self.output_shape, None, "sparse")
        self._taps = None
        self._pinned = None
        self.coverage = (0, 0)
        self.handoff_modes = {"device_edit": 0, "fast": 0, "host": 0}     # which form each training step's hand-off took
        self.phase_ms = {}         # host phases of the last RoI hand-off in ms, the reference's names (denet_sparse.py:127-161)

    # the host-side views of the edited RoI list. After a device-side edit (_device_edit) they are produced by the first reader -
    # the detection layer's get_target, a few layers on, while the device runs the gather and the head
    def _resolve_edit(self):
        job = self.__dict__.pop("_lazy_edit", None)
        if job is not None:
            job()

    def _lazy_view(name):
        def get(self):
            self._resolve_edit()
            return getattr(self, name)

        def put(self, v):
            self.__dict__.pop("_lazy_edit", None)        # an explicit list replaces whatever was pending
            setattr(self, name, v)
        return property(get, put)

    sample_pr, sample_boxes, sample_bbox_f32 = _lazy_view("_sample_pr"), _lazy_view("_sample_boxes"), _lazy_view("_sample_bbox_f32")
    del _lazy_view

    @staticmethod
    def parse_desc(layers, name, tags, params):
        if name != "DNS":
            return False
        # tag I (this build's own): bilinear taps. Without it the constructor is called exactly as the reference calls its own
        extra = {"tap_rule": TAP_BILINEAR} if "I" in tags else {}
        layers.append(DeNetSparseLayer(layers, params.get(0, 3), params.get(1, 4), params.get(2, 0.01),
                                       params.get(3, 0.1), params.get(4, 0), params.get(5, 1.0), not "G" in tags, **extra))
        return True

    # ---- reference list-of-tuples view --------------------------------------------------------------------
    @property
    def sample_bbox_list(self):
        return [[(float(p), tuple(bx)) for p, bx in zip(pr.tolist(), boxes.tolist())]
                for pr, boxes in zip(self.sample_pr, self.sample_boxes)]

    @staticmethod
    def _from_lists(sample_bboxs):
        prs, boxes = [], []
        for samples in sample_bboxs:
            prs.append(numpy.array([s[0] for s in samples], dtype=numpy.float64).reshape(-1))
            boxes.append(numpy.array([s[1] for s in samples], dtype=numpy.float64).reshape(-1, 4))
        return prs, boxes

    # ---- corner detector -> sample boxes ------------------------------------------------------------------
    def _device_samples(self, store_shared=False, raw_only=False):
        """GPU RoI proposal + ONE device->host copy of its packed result (boxes, |d|, counts)"""
        import torch
        cl = self.corner_layer
        assert cl.corner_pr is not None, "run the model forward up to the corner layer first"
        # the reference's phases (denet_sparse.py:127-145): "model" = the corner function (here: queueing the proposal kernels
        # and waiting until the device has run the forward pass up to the corner map + the proposal), "build" = the host
        # part of build_samples (here only its epilogue: libm score, box arithmetic, optional clustering)
        timer = common.Timer()
        # the opt-in device clustering (read here, where the step's proposal is queued): the 10 * sn^2 candidates stay in a
        # device staging buffer and the packed result is the clustered, sn^2 wide list - from here on an ordinary proposal
        self._dev_clustered = self._cluster_on_device()
        B, S = self.batch_size, self._list_width()
        words = B * S * 5 + B
        if getattr(self, "_res_dev", None) is None or self._res_dev.numel() != words:
            # (one pair of buffers per width: a clustering layer whose mode changes between steps goes back to the pair it had)
            sets = self.__dict__.setdefault("_res_sets", {})
            if words not in sets:
                sets[words] = (torch.empty(words, dtype=torch.int32, device="cuda"), torch.empty(words, dtype=torch.int32).pin_memory())
            self._res_dev, self._res_host = sets[words]
            self._res_counts = None
        r = self._res_dev
        box = r[:B * S * 4].view(B, S, 4)
        absd = r[B * S * 4:B * S * 5].view(torch.float32).view(B, S)
        count = r[B * S * 5:]
        if self._dev_clustered:
            P = self.proposal_count
            st = self.__dict__.get("_stage_dev")
            if st is None:
                st = self._stage_dev = torch.empty(B * P * 5 + B, dtype=torch.int32, device="cuda")
            staged = (st[:B * P * 4].view(B, P, 4), st[B * P * 4:B * P * 5].view(torch.float32).view(B, P), st[B * P * 5:])
            ops.build_samples(cl.corner_pr, float(self.corner_threshold), P, self.corner_max, int(self.local_max), out=staged)
            ops.cluster_samples_device(*staged, float(self.nms_threshold), S, cl.height, cl.width, out=(box, absd, count))
        else:
            ops.build_samples(cl.corner_pr, float(self.corner_threshold), S, self.corner_max, int(self.local_max),
                              out=(box, absd, count))
        if store_shared:
            cl.sample_shared = cl.conv.output.data
        self._res_host.copy_(r, non_blocking=True)
        # everything the hand-off can settle without the proposal is settled BEFORE the wait (the device stands idle from the
        # moment the copy lands until the gather is queued): the checks of the short forms, the gather's output buffers
        ready = self._short_handoff_ready() if raw_only else None
        if raw_only and get_train() and self.tap_rule != TAP_BILINEAR:
            self._gather_pre = ops.sparse_fwd_buffers(self.batch_size * self.sample_count, self.grid_size, self.output.cp)
        # ... and while it waits (the device is a whole backbone behind), the host repeats a dry run of the fast form's native call
        # every quarter of a millisecond: the call finds its code, tables and the generator stretch in cache when the proposal lands
        warm = (lambda: self._warm_fast_handoff(ready)) if (raw_only and get_train() and _RH.WARM_PERIOD > 0) else None
        ops.wait_stream(idle=warm, period=_RH.WARM_PERIOD)
        # from here to the upload of the bbox array the device stands idle: numpy views of the pinned buffer made once, every
        # property of the counts computed once
        timer.mark()
        hc = self.__dict__.get("_res_counts")
        if hc is None or hc.size != B:
            hc = self._res_counts = self._res_host.numpy()[B * S * 5:]
        tot = int(hc.sum())
        self._raw_samples = None
        self._deferred = None
        self.proposed_total = getattr(self, "proposed_total", 0) + tot      # (what regime a run was in: bench.py)
        self.proposed_steps = getattr(self, "proposed_steps", 0) + 1
        if raw_only and self._short_handoff(hc, tot, ready):
            # the bbox array is on its way (edited on the device, or by ONE native host call); everything else of the host's share
            # - the Python-side list, the generator's state - waits for its first reader
            self._deferred = timer
            self._log_get_samples(timer)
            return None, None
        return self._finish_samples(timer, raw_only)

    _dev_clustered = False         # the proposal in flight was clustered on the device (set by _device_samples)

    def _cluster_on_device(self):
        """this layer clusters and the opt-in device form applies: mode on, a threshold the closed form covers, a device"""
        return self.cluster and ops.CLUSTER_DEVICE and 0.0 <= self.nms_threshold < 1.0 and self._on_device()

    def _list_width(self):
        """rows per image of the packed result the device hands over: sn^2, or the 10 * sn^2 candidates the host will cluster"""
        return self.sample_count if self._dev_clustered else self.proposal_count

    def _finish_samples(self, timer, raw_only, log=True):
        """host epilogue of the proposal: sample tuples from the packed result in the pinned buffer"""
        import torch
        cl = self.corner_layer
        B, S = self.batch_size, self._list_width()
        h = self._res_host
        hcount = h[B * S * 5:]
        if int(hcount.sum()) == 0:        # cold detector: nothing proposed
            empty_pr, empty_bx = numpy.zeros((0,)), numpy.zeros((0, 4))
            if log:
                self._log_get_samples(timer)
            return [empty_pr] * B, [empty_bx] * B
        hbox = h[:B * S * 4].view(B, S, 4)
        habsd = h[B * S * 4:B * S * 5].view(torch.float32).view(B, S)
        # two buffers in turn: the rows of a step are read until its detection targets are built, i.e. into the next forward pass
        ring = self.__dict__.setdefault("_finish_ring", [None, None])
        self._finish_turn = 1 - getattr(self, "_finish_turn", 0)
        out = ops.samples_finish_host(hbox, habsd, hcount, cl.height, cl.width, out=ring[self._finish_turn])
        ring[self._finish_turn] = out
        raw = out.numpy()
        hcount = hcount.numpy()
        if self.cluster and not self._dev_clustered:
            raw, hcount = ops.cluster_samples_host(raw, hcount, self.nms_threshold, self.sample_count)
        self._raw_samples = (raw, hcount)
        if log:
            self._log_get_samples(timer)
        if raw_only:
            return None, None
        samples = raw.astype(numpy.float64)
        counts = [int(c) for c in hcount]
        prs = [samples[b, :counts[b], 0] for b in range(B)]
        boxes = [samples[b, :counts[b], 1:5] for b in range(B)]
        return prs, boxes

    def _log_get_samples(self, timer):
        timer.mark()
        # phase_ms: last value of every host phase of the RoI hand-off, under the reference's names
        self.phase_ms["get_samples"] = timer.current_ms()
        self.phase_ms["get_samples.model"] = timer.delta_ms(0)
        self.phase_ms["get_samples.build"] = timer.delta_ms(1)
        if logging.verbose_enabled():
            logging.verbose("Took %i ms to get_samples (%i model, %i build, %i max corners) "
                            % (timer.current_ms(), timer.delta_ms(0), timer.delta_ms(1), self.corner_max))

    def get_samples(self, data_x, train=False, store_shared=False):
        """list[B] of list[(pr, (x0, y0, x1, y1))], the return shape of c_code.build_samples
        (denet_sparse.cc:587-592). Uses the corner map of the forward pass in flight."""
        prs, boxes = self._device_samples(store_shared)
        return [[(p, tuple(bx)) for p, bx in zip(pr.tolist(), bxs.tolist())] for pr, bxs in zip(prs, boxes)]

    def get_bbox_array(self, sample_bboxs):
        """build_bbox_array (denet_sparse.cc:670-699): bbox[b, i//sn, i%sn] = box i; the rest stays 0"""
        _, boxes = self._from_lists(sample_bboxs)
        return self._bbox_array(boxes)

    def _bbox_array(self, boxes):
        bboxs = numpy.zeros((self.batch_size, self.sample_num, self.sample_num, 4), dtype=numpy.float32)
        flat = bboxs.reshape(self.batch_size, self.sample_count, 4)
        for b, bx in enumerate(boxes):
            if len(bx) > 0:
                flat[b, :len(bx)] = bx
        return bboxs

    def set_samples(self, sample_bboxs):
        self.sample_pr, self.sample_boxes = self._from_lists(sample_bboxs)
        return self._upload_boxes()

    def _upload_boxes(self):
        import torch
        bboxs = self._bbox_array(self.sample_boxes)
        if self._pinned is None:
            self._pinned = torch.empty((self.batch_size * self.sample_count, 4), dtype=torch.float32).pin_memory()
        self._pinned.copy_(torch.from_numpy(bboxs.reshape(-1, 4)))
        self.sample_bbox = self._pinned.cuda(non_blocking=True)
        self.sample_bbox_f32 = bboxs.reshape(self.batch_size, self.sample_count, 4)
        return bboxs

    def edit_samples(self, prs, boxes, metas):
        """training-time RoI list editing (denet_sparse.py:184-201), call for call on the stdlib generator:
        random.sample when the detector produced too many boxes, then 4 uniform draws per random box in the order
        x0, y0, x1, y1, then ground truth written over the tail of the list. Draws of consecutive images that need
        no trimming are taken from the generator in one vectorised batch (same stream, same order)."""
        total_cover = total_bbox = 0
        S = self.sample_count
        n_keep = S - math.floor(self.random_sample * S)
        B = len(metas)
        out_pr = [None] * B
        out_boxes = [None] * B
        mirror = PyRandomMirror()

        def fill(first, last, kept):
            """random boxes for images first..last-1 (none of them trims): one bulk draw, split in image order"""
            ks = [S - len(kept[b][1]) for b in range(first, last)]
            r = mirror.doubles(4 * sum(ks)).reshape(-1, 4)
            # random.uniform(a, b) = a + (b - a) * random()
            x0 = 0.0 + (1.0 - 0.0) * r[:, 0]
            y0 = 0.0 + (1.0 - 0.0) * r[:, 1]
            x1 = x0 + (1.0 - x0) * r[:, 2]
            y1 = y0 + (1.0 - y0) * r[:, 3]
            rnd = numpy.stack([x0, y0, x1, y1], axis=1)
            off = 0
            for b, k in zip(range(first, last), ks):
                pr, bx = kept[b]
                if k > 0:
                    bx = numpy.concatenate([bx, rnd[off:off + k]], axis=0) if len(bx) else rnd[off:off + k].copy()
                    pr = numpy.concatenate([pr, numpy.zeros(k)]) if len(pr) else numpy.zeros(k)
                    off += k
                else:
                    bx, pr = bx.copy(), pr.copy()
                if self.sample_gt:
                    gt = metas[b]["bbox"]
                    n = len(gt)
                    if n > 0:
                        # sample_bboxs[b][-(index+1)] = (1.0, bbox): ground truth k lands at position -(k+1)
                        bx[S - n:] = numpy.asarray(gt, dtype=numpy.float64)[::-1]
                        pr[S - n:] = 1.0
                out_pr[b], out_boxes[b] = pr, bx

        kept = {}
        run_start = 0
        for b, meta in enumerate(metas):
            pr, bx = prs[b], boxes[b]
            if self.log_coverage:
                cover = 0
                for meta_bbox in meta["bbox"]:
                    for sample_bbox in bx.tolist():
                        if common.overlap_iou(meta_bbox, sample_bbox) > 0.5:
                            cover += 1
                            break
                total_cover += cover
                total_bbox += len(meta["bbox"])
            if len(bx) > n_keep:
                # the trim of image b happens after the random boxes of images < b were drawn
                fill(run_start, b, kept)
                run_start = b
                keep = mirror.sample(len(bx), n_keep)             # same draws as random.sample(list, n)
                pr, bx = pr[keep], bx[keep]
            kept[b] = (pr, bx)
        fill(run_start, B, kept)
        mirror.push()
        self.coverage = (total_cover, total_bbox)
        return out_pr, out_boxes

    def begin_step(self, metas):
        """host work of the RoI editing that does not depend on the detector, done at the start of the forward pass
        while the GPU is busy with the backbone instead of inside the GPU-idle hand-off: ground-truth arrays and the
        snapshot of the stdlib generator (re-validated with PyRandomMirror.fresh() before use)"""
        B = self.batch_size
        self._resolve_edit()              # (a list of the previous step nobody read)
        self._check_device_edit_status()
        prep = {"metas": metas, "mirror": PyRandomMirror()}
        if self.sample_gt:
            gts = [numpy.asarray(m["bbox"], dtype=numpy.float64).reshape(-1, 4) for m in metas]
            off = numpy.zeros(len(metas) + 1, dtype=numpy.int32)
            numpy.cumsum([len(g) for g in gts], out=off[1:])
            prep["off"] = off
            prep["gt"] = numpy.ascontiguousarray(numpy.concatenate(gts, axis=0)) if off[-1] > 0 else numpy.zeros((1, 4))
        else:
            prep["off"], prep["gt"] = numpy.zeros(len(metas) + 1, dtype=numpy.int32), numpy.zeros((1, 4))
        self._prep = prep
        self._prefetch = None
        self._dev_edit = None
        if get_train() and self._native_edit_ok(metas) and _RH.PREFETCH_RANDOM:
            self._prefetch_random()
            # (the device-side editing reads an sn^2 wide hand-off list: no clustering, or clustering on the device)
            if _RH.DEVICE_EDIT and self._on_device() and (not self.cluster or self._cluster_on_device()):
                self._upload_for_device_edit(metas, prep)

    _ON_DEVICE = None

    @staticmethod
    def _on_device():
        # asked inside the RoI hand-off, where the device stands idle: torch.cuda.is_available() queries the runtime's device count on
        # every call (tens of microseconds), the answer cannot change
        if DeNetSparseLayer._ON_DEVICE is None:
            import torch
            DeNetSparseLayer._ON_DEVICE = bool(torch.cuda.is_available())
        return DeNetSparseLayer._ON_DEVICE

    def edit_samples_native(self, det, cnt, metas, out_f32, defer_push=False):
        """edit_samples for the whole batch in one native host call (denet_host_edit_samples): same generator
        stream, same values. det [B,S,5] float32 rows (pr, box) of the detector, cnt [B]; out_f32 [B*S,4] float32
        receives the array build_bbox_array would produce. Returns (pr [B,S], boxes [B,S,4]) as float64."""
        det = numpy.ascontiguousarray(det, dtype=numpy.float32)
        cnt = numpy.ascontiguousarray(cnt, dtype=numpy.int32)
        prep = getattr(self, "_prep", None)
        if prep is None or prep["metas"] is not metas:
            self.begin_step(metas)
            prep = self._prep
        self._prep = None
        pf = self.__dict__.pop("_prefetch", None)
        done = None
        if pf is not None and pf["mirror"].fresh():
            done = self._native_edit_stream(pf, det, cnt, prep, out_f32)
        if done is not None:
            out_pr, out_box, mirror = done
        else:
            mirror = prep["mirror"] if prep["mirror"].fresh() else PyRandomMirror()
            out_pr, out_box = self._native_edit(mirror, det, cnt, prep, out_f32)
        if defer_push:
            self._pending_push = mirror      # handed back to the stdlib generator once the gather is queued
        else:
            mirror.push()
        return out_pr, out_box

    def _edit_and_upload_native(self, metas):
        """the ordinary path: editing in one native host call, then the upload"""
        import torch
        B, S = self.batch_size, self.sample_count
        if self._pinned is None:
            self._pinned = torch.empty((B * S, 4), dtype=torch.float32).pin_memory()
        if self._raw_samples is not None:
            det, cnt = self._raw_samples
        else:
            det, cnt = numpy.zeros((B, S, 5), dtype=numpy.float32), numpy.zeros(B, dtype=numpy.int32)
        f32 = self._pinned.numpy()
        out_pr, out_box = self.edit_samples_native(det, cnt, metas, f32, defer_push=True)
        self.sample_pr, self.sample_boxes = list(out_pr), list(out_box)
        self.sample_bbox = self._pinned.cuda(non_blocking=True)
        self.sample_bbox_f32 = f32.reshape(B, S, 4)
        self.handoff_modes["host"] += 1

    def _native_edit_ok(self, metas):
        """random.sample's pool branch (n <= setsize) covers every possible trim, and no coverage logging"""
        S = self.sample_count
        k = S - math.floor(self.random_sample * S)
        setsize = 21 + (4 ** math.ceil(math.log(k * 3, 4)) if k > 5 else 0)
        return S <= setsize and not self.log_coverage and len(metas) == self.batch_size

    def get_target(self, model, data_x, metas):
        timer = common.Timer()
        native = self._native_edit_ok(metas)
        if self.__dict__.get("_prep") is None or self._prep["metas"] is not metas:
            self._dev_edit = None            # prepared for another batch
        prs, boxes = self._device_samples(raw_only=native)
        timer.mark()
        if native and self._deferred is not None:
            self._deferred = None            # edited on the device (_device_edit): the gather is not waiting for anything
        elif native:
            self._edit_and_upload_native(metas)
        else:
            self.sample_pr, self.sample_boxes = self.edit_samples(prs, boxes, metas)
            self._upload_boxes()
            self.handoff_modes["host"] += 1
        timer.mark()
        # the reference logs get_bbox_array and set_samples separately (denet_sparse.py:148-161); here the RoI editing
        # writes the bbox array straight into the pinned upload buffer, so the two are one phase
        self.phase_ms["set_samples"] = timer.delta_ms(1)
        self.phase_ms["get_target"] = timer.current_ms()
        if logging.verbose_enabled():
            logging.debug("Took %i ms to set_samples" % timer.delta_ms(1))
        return None

    def export_json(self):
        json = super().export_json()
        json.update({"gridSize": self.grid_size, "sampleNum": self.sample_num, "sampleGT": self.sample_gt,
                     "localMax": self.local_max, "cornerThreshold": self.corner_threshold,
                     "randomSample": self.random_sample, "nmsThreshold": self.nms_threshold, "version": self.version})
        if self.tap_rule != TAP_THEANO:      # (a default layer's dictionary stays the reference's, key for key)
            json["tapRule"] = self.tap_rule
        return json

    # ---- execution ----------------------------------------------------------------------------------------
    def forward(self, ctx):
        cl = self.corner_layer
        if not get_train():
            # inference (denet_detect.py:369-375): RoIs straight from the corner detector, no editing
            self.sample_pr, self.sample_boxes = self._device_samples(store_shared=True)
            self._upload_boxes()
        if get_train() or cl.sample_shared is None:
            fmap, coff, F = cl.sample_map()
        else:
            fmap, coff, F = cl.sample_shared, cl.corner_num, cl.sample_feat
        assert self.sample_bbox is not None, "set_samples() must run before the sparse layer"
        side_sort = get_train() and os.environ.get("DENET_SIDE_SORT", "1") == "1"
        fm = fmap.shape
        self._sorted_ev = None
        if self.tap_rule == TAP_BILINEAR:
            self.__dict__.pop("_gather_pre", None)           # (the nearest rules' buffers: this rule keeps four cells and weights per tap)
            out, self._taps, self._wts = ops.sparse_bilinear_fwd(fmap, self.sample_bbox, coff, F, self.sample_count, self.grid_size,
                                                                 self.output.cp, keep=get_train())
            if side_sort:
                self._sorted_ev = ops.sparse_bilinear_sort_async(self._taps, fm[0], fm[1], fm[2], self.sample_count, self.grid_size)
        else:
            out, self._taps = ops.sparse_fwd(fmap, self.sample_bbox, coff, F, self.sample_count, self.grid_size,
                                             self.output.cp, self.tap_rule, buffers=self.__dict__.pop("_gather_pre", None))
            if side_sort:
                self._sorted_ev = ops.sparse_sort_async(self._taps, fm[0], fm[1], fm[2], self.sample_count, self.grid_size)
        self.output.data = out.view(self.batch_size, self.sample_num, self.sample_num, self.output.cp)
        mirror = self.__dict__.pop("_pending_push", None)
        if mirror is not None:
            mirror.push()

    def backward(self, ctx):
        cl = self.corner_layer
        dconv = cl.alloc_dconv(zero=False)
        dy = self.output.grad.view(-1, self.output.cp)
        if self.tap_rule == TAP_BILINEAR:
            ops.sparse_bilinear_bwd(dy, self._taps, self._wts, dconv, cl.corner_num, cl.sample_feat, self.sample_count, self.grid_size,
                                    cl.corner_num + cl.sample_feat, presorted=getattr(self, "_sorted_ev", None))
            return
        ops.sparse_bwd(dy, self._taps, dconv, cl.corner_num, cl.sample_feat, self.sample_count, self.grid_size,
                       cl.corner_num + cl.sample_feat, presorted=getattr(self, "_sorted_ev", None))
