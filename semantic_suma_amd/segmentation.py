"""Semantic front end: the device side of RangeNet++'s inference around a PyTorch segmentation network.

The reference's reader (src/io/KITTIReader.cpp:172-200) hands each scan to ``RangenetAPI::infer`` (TensorRT), which
projects it to a range image, runs the network and returns N x 20 per-point class scores; the reader then takes the
argmax and maps the winner through the network's label map.  TensorRT does not exist on an MI355X, so here the network
is the caller's PyTorch model, and the two data-parallel stages around it are HIP kernels (csrc/k_semantic.hip):

    project(points)            N x (x, y, z, remission) -> input [1, 5, H, W] fp32 (range, x, y, z, remission),
                               normalised (v - mean) / std; also keeps pixel[N] and proj_idx[H, W]
    unproject(scores, logits)  planar [1, C, H, W] fp32 scores -> per-point (labels[N], probs[N]) by the reference's
                               argmax rule (the last maximum wins, all-negative scores give (0, 0), NaN never wins);
                               knn=semantic_knn(): RangeNet++'s KNN post-processing instead (csrc/k_semantic_knn.hip),
                               a vote among the points nearest in range around each point's pixel
    process_scan(mapping, ...) project -> model(input) -> SurfelMapping.processScanScores: the back-projection and K1-K3
                               run on the pipeline's preprocessing stream behind an event, without a host synchronisation

Projection convention (RangeNet++'s, the one its networks are trained on): depth = |p|, yaw = -atan2(y, x),
pitch = asin(z / depth), u = 0.5 (yaw / pi + 1) W, v = (1 - (pitch + |fov_down|) / fov) H with
fov = |fov_up| + |fov_down|; floor, then clamp to [0, W-1] x [0, H-1].  Row 0 of the network's image is the TOP (highest
pitch), the opposite of the frames' vertex maps.  A point with a non-finite coordinate or zero range is not projected;
the nearest point wins its pixel, equal ranges go to the lower point index.  The exact fp32 operation order is
stated in csrc/k_semantic.hip.

Streams: the kernels and the model run on the context's stream (``torch.cuda.ExternalStream(ctx.stream)``), which first
waits for the caller's current torch stream; before a call returns, the caller's current stream waits for the
context's stream again.  That wait is what keeps the tensors the kernels and the pipeline read alive: a block freed
after the call is reused by work on the caller's stream, which now runs behind everything the call enqueued -- for
process_scan that includes the pipeline's preprocessing, which its ctx stream joins before the map update.  (No
``record_stream`` on the context's stream: the caching allocator would record events on it after the context, and
with it the stream, may be gone.)  Tensors made on other streams follow torch's usual multi-stream rules.

KNN post-processing (RangeNet++, Milioto et al., IROS 2019, section III-D; opt-in, ``knn=semantic_knn()``): a point
hidden behind a nearer one in its pixel otherwise takes that one's class, so at every depth edge the foreground's
class bleeds onto the background.  With ``knn`` each point's label is voted by the k candidates nearest in range among
its pixel and the search x search pixels around it (weighted by an inverted Gaussian of the offset, class 0 and
candidates farther than ``cutoff`` do not vote).  The arithmetic is stated in csrc/k_semantic_knn.hip.

The means and stds have no defaults: they belong to the trained model (RangeNet++ ships them in its arch_cfg.yaml
``sensor: img_means / img_stds``).  The label map defaults to SemanticKITTI's learning_map_inv.  No weights ship here.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import kitti
from .core import Context, SumaError, SurfelMapping
from .types import SEM_CHANNELS, SEM_MAX_CLASSES, SemanticKnnParams, SemanticParams


def semantic_params(width: int, height: int, fov_up: float, fov_down: float, means, stds, n_classes: int = 20,
                    label_map=None) -> SemanticParams:
    """suma_semantic_params from a model's sensor config.  fov in degrees; means / stds: 5 values each in the channel
    order (range, x, y, z, remission); label_map: class index -> reported label id (sequence or dict), default
    kitti.LEARNING_MAP_INV."""
    means, stds = list(means), list(stds)
    if len(means) != SEM_CHANNELS or len(stds) != SEM_CHANNELS:
        raise ValueError(f"means / stds need {SEM_CHANNELS} values (range, x, y, z, remission)")
    if label_map is None:
        label_map = kitti.LEARNING_MAP_INV
    if isinstance(label_map, dict):
        label_map = [label_map.get(j, 0) for j in range(n_classes)]
    label_map = list(label_map)
    if len(label_map) > SEM_MAX_CLASSES:
        raise ValueError(f"label_map: more than {SEM_MAX_CLASSES} classes")
    sp = SemanticParams(width=width, height=height, fov_up=fov_up, fov_down=fov_down, n_classes=n_classes)
    for c in range(SEM_CHANNELS):
        sp.means[c], sp.stds[c] = means[c], stds[c]
    for j, v in enumerate(label_map):
        sp.label_map[j] = int(v)
    return sp


def semantic_knn(search: int = 5, k: int = 5, sigma: float = 1.0, cutoff: float = 1.0) -> SemanticKnnParams:
    """suma_semantic_knn, RangeNet++'s published defaults: a search x search window (odd, 1 .. 9), k voters
    (1 .. search^2), the Gaussian's sigma (> 0) and the range cutoff in metres (<= 0: none).  The library checks them."""
    return SemanticKnnParams(search=search, k=k, sigma=sigma, cutoff=cutoff)


def _check_one_hip_runtime():
    """torch and libsuma_hip.so must share ONE HIP runtime: stream and event handles of one are meaningless to another.
    Both name it libamdhip64.so.7; whichever loads first serves both -- unless the library was loaded before torch, when
    torch's own copy can come up beside it."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    if len(paths) > 1:
        raise SumaError("two HIP runtimes are loaded (" + ", ".join(sorted(paths)) + "): import torch before "
                        "semantic_suma_amd.core.lib() is first called")


class SemanticFrontEnd:
    """Range-image projection and score back-projection for one network geometry on one context (or pipeline)."""

    def __init__(self, ctx_or_mapping, semantic_params: SemanticParams):
        if isinstance(ctx_or_mapping, SurfelMapping):
            self.mapping, self.ctx = ctx_or_mapping, ctx_or_mapping.ctx
        elif isinstance(ctx_or_mapping, Context):
            self.mapping, self.ctx = None, ctx_or_mapping
        else:
            raise TypeError("SemanticFrontEnd needs a core.Context or a core.SurfelMapping")
        _check_one_hip_runtime()
        self.sp = semantic_params
        self.L = self.ctx.L
        self.width, self.height = int(semantic_params.width), int(semantic_params.height)
        self.n_classes = int(semantic_params.n_classes)
        self.pixel = None     # int32 [N]: pixel of every point of the last projection, -1 = not projected
        self.proj_idx = None  # int32 [H, W]: winning point of every pixel, -1 = empty
        self.points = None    # float32 [N, 4]: the points of the last projection (the KNN back-projection reads them)
        self.input = None     # fp32 [1, 5, H, W]
        self._event = None

    def _stream(self, device):
        return torch.cuda.ExternalStream(self.ctx.stream, device=device)

    def _points(self, points):
        if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32):
            raise TypeError("points: a float32 CUDA tensor of N x 4 (x, y, z, remission)")
        if points.dim() != 2 or points.shape[1] != 4:
            raise ValueError(f"points: shape {tuple(points.shape)}, expected N x 4")
        return points.contiguous()

    def _scores(self, scores):
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32):
            raise TypeError("scores: a float32 CUDA tensor [1, C, H, W] or [C, H, W]")
        shape = (self.n_classes, self.height, self.width)
        if tuple(scores.shape[-3:]) != shape or scores.dim() not in (3, 4) or (scores.dim() == 4 and scores.shape[0] != 1):
            raise ValueError(f"scores: shape {tuple(scores.shape)}, expected [1, {shape[0]}, {shape[1]}, {shape[2]}]")
        return scores.contiguous()

    def _project_on(self, ext, points):
        n = points.shape[0]
        dev = points.device
        inp = torch.empty((1, SEM_CHANNELS, self.height, self.width), dtype=torch.float32, device=dev)
        pixel = torch.empty(n, dtype=torch.int32, device=dev)
        proj_idx = torch.empty((self.height, self.width), dtype=torch.int32, device=dev)
        self.ctx.check(self.L.suma_semantic_project(self.ctx.h, C.byref(self.sp), C.c_void_p(points.data_ptr()), n,
                                                    C.c_void_p(inp.data_ptr()), C.c_void_p(pixel.data_ptr()),
                                                    C.c_void_p(proj_idx.data_ptr())),
                       "suma_semantic_project")
        self.input, self.pixel, self.proj_idx, self.points = inp, pixel, proj_idx, points
        return inp

    def project(self, points):
        """points: float32 CUDA [N, 4] (x, y, z, remission) -> input [1, 5, H, W]; keeps pixel / proj_idx"""
        points = self._points(points)
        cur = torch.cuda.current_stream(points.device)
        ext = self._stream(points.device)
        ext.wait_stream(cur)
        inp = self._project_on(ext, points)
        cur.wait_stream(ext)
        return inp

    def unproject(self, scores, logits: bool = False, pixel=None, knn: SemanticKnnParams = None, points=None,
                  proj_idx=None):
        """planar fp32 scores [1, C, H, W] -> (labels[N], probs[N]) float32 for the points of the last projection
        (or of ``pixel``); logits=True applies a softmax over C first.  ``knn`` (semantic_knn()): RangeNet++'s KNN
        post-processing, which also reads the projection's points and proj_idx (pass ``points`` / ``proj_idx`` with
        ``pixel``)"""
        scores = self._scores(scores)
        if pixel is None:
            pixel, points_, proj_idx_ = self.pixel, self.points, self.proj_idx
            points = points_ if points is None else points
            proj_idx = proj_idx_ if proj_idx is None else proj_idx
        if pixel is None:
            raise ValueError("unproject: no projection yet (call project first or pass pixel)")
        if knn is not None and (points is None or proj_idx is None):
            raise ValueError("unproject: knn needs the projection's points and proj_idx with an explicit pixel")
        n = pixel.shape[0]
        dev = scores.device
        labels = torch.empty(n, dtype=torch.float32, device=dev)
        probs = torch.empty(n, dtype=torch.float32, device=dev)
        cur = torch.cuda.current_stream(dev)
        ext = self._stream(dev)
        ext.wait_stream(cur)
        if knn is None:
            self.ctx.check(self.L.suma_semantic_unproject(self.ctx.h, C.byref(self.sp), C.c_void_p(scores.data_ptr()),
                                                          int(bool(logits)), C.c_void_p(pixel.data_ptr()), n,
                                                          C.c_void_p(labels.data_ptr()), C.c_void_p(probs.data_ptr())),
                           "suma_semantic_unproject")
        else:
            points = self._points(points)
            if points.shape[0] != n or proj_idx.numel() != self.width * self.height:
                raise ValueError("unproject: points / pixel / proj_idx are not of one projection")
            self.ctx.check(self.L.suma_semantic_unproject_knn(self.ctx.h, C.byref(self.sp), C.byref(knn),
                                                              C.c_void_p(points.data_ptr()),
                                                              C.c_void_p(scores.data_ptr()), int(bool(logits)),
                                                              C.c_void_p(pixel.data_ptr()),
                                                              C.c_void_p(proj_idx.data_ptr()), n,
                                                              C.c_void_p(labels.data_ptr()),
                                                              C.c_void_p(probs.data_ptr())),
                           "suma_semantic_unproject_knn")
        cur.wait_stream(ext)
        return labels, probs

    def process_scan(self, mapping, points, model, fixed_iterations: int = 0, logits: bool = False,
                     knn: SemanticKnnParams = None):
        """SurfelMapping.processScan with the labels of ``model``: project -> model(input) -> the pipeline's scores
        entry (its KNN form with ``knn``).  The model runs on the context's stream; the pipeline's preprocessing waits
        for it on the device."""
        mapping = self.mapping if mapping is None else mapping
        if not isinstance(mapping, SurfelMapping):
            raise TypeError("process_scan needs a core.SurfelMapping")
        points = self._points(points)
        dev = points.device
        cur = torch.cuda.current_stream(dev)
        ext = self._stream(dev)
        ext.wait_stream(cur)
        inp = self._project_on(ext, points)
        with torch.cuda.stream(ext):
            scores = self._scores(model(inp))
            event = torch.cuda.Event()
            event.record(ext)
        mapping.processScanScores(self.sp, points.data_ptr(), scores.data_ptr(), self.pixel.data_ptr(), points.shape[0],
                                  logits=logits, producer_event=event.cuda_event, fixed_iterations=fixed_iterations,
                                  knn=knn, d_proj_idx=self.proj_idx.data_ptr())
        self._event = event  # the preprocessing stream's wait may still be pending: keep the event until the next scan
        # the pipeline's ctx stream has passed its preprocessing once it has passed this scan's map update
        if mapping.ctx.h.value != self.ctx.h.value:
            cur.wait_stream(torch.cuda.ExternalStream(mapping.ctx.stream, device=dev))
        cur.wait_stream(ext)
        return scores
