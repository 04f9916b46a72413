"""Sparse 3-D FPN backbone: same module tree / parameter names as
SparseConvNet/sparseconvnet/fpn_net.py:12-137 (so `backbone.*` checkpoint keys load unchanged),
same outputs as its forward_fpn (:168-265), executed by the HIP ops of libd3d_hip.so.

Execution switches that do not change any returned tensor (SIDE_STREAMS below is a third):
  * fuse_adds     -- residual / lateral additions run in the epilogue of the producing
                     convolution instead of a separate AddTable / add_feature_planes pass;
  * skip_unused   -- the top-down levels whose outputs nothing consumes for the configured
                     fpn_scales_from_top / roi_scales_from_top (m_ups[5..7] for fpn432) are not
                     computed; the reference computes and discards them (fpn_net.py:186-196).
"""
import numpy as np
import os

import torch
import torch.nn as nn

from . import modules as scn
from ..timeline import mark as _tmark

SIDE_STREAMS = True     # GPU inputs: the geometry of the pyramid on side streams (_forward_async_geometry); False: the
                        # one-stream pass (tests)
_GEO_STREAMS = {}   # (device, caller's stream) -> side streams
# priority of the side streams: 0 = normal (default), -1 = high (geometry ahead of the convolutions).  Measured in pairs on
# two boxes: 4.80 (high) against 4.82 ms (normal) per building on one, 5.28-5.37 against 4.86-4.95 on the other -- high
# priority buys nothing where it works and costs 8 % where the queue scheduler lets the geometry kernels hold back the
# caller's stream
_SIDE_PRIORITY = int(os.environ.get("D3D_SIDE_PRIORITY", "0"))
# fp32 inference with fuse_adds on the GPU: the convolutions of the top-down path that do not depend on one another --
# the lateral 1x1x1 shortcuts, the merged maps, the 2-D projections -- run as three grouped calls (scn.conv_group) around
# the chain BatchNorm statistics -> deconvolution, instead of in line between its links.  Same kernels' bodies on the same
# data (bit-identical); D3D_CONV_GROUP=0 restores the one-by-one order (A/B runs).
GROUP_CONVS = os.environ.get("D3D_CONV_GROUP", "1") != "0"


def _is_gpu_input(net0):
    return isinstance(net0, (list, tuple)) and len(net0) > 1 and torch.is_tensor(net0[1]) and net0[1].is_cuda


def _geometry_stream(main):
    """-> (geometry stream, its reusable events, plan stream) of the caller's stream"""
    key = (main.device.index, main.cuda_stream)
    st = _GEO_STREAMS.get(key)
    if st is None:
        st = _GEO_STREAMS[key] = (torch.cuda.Stream(device=main.device, priority=_SIDE_PRIORITY),
                                  [torch.cuda.Event() for _ in range(2)],
                                  torch.cuda.Stream(device=main.device, priority=_SIDE_PRIORITY))
    return st


class _RowsToBf16(torch.autograd.Function):
    """fp32 rows -> bf16 rows in one launch (d3d_rows_to_bf16); the gradient goes back widened to fp32"""

    @staticmethod
    def forward(ctx, f):
        return scn.SCN.rows_to_bf16(f, f.shape[1])

    @staticmethod
    def backward(ctx, grad):
        return grad.float()


def _rows_to_bf16(f):
    """an fp32 map's rows for bf16 heads (round to nearest even, as .to(torch.bfloat16))"""
    if f.is_cuda and f.dim() == 2 and f.shape[1] % 8 == 0:
        return _RowsToBf16.apply(f)
    return f.to(torch.bfloat16)


class FPN_Net(torch.nn.Module):
    def __init__(self, full_scale, dimension, raw_elements, reps, nPlanesF, nPlaneM, residual_blocks,
                 fpn_scales_from_top, roi_scales_from_top, downsample, rpn_map_sizes,
                 rpn_3d_2d_selector, leakiness=0, voxel_scale=None, bn_momentum=0.9,
                 track_running_stats=True, fuse_adds=True, skip_unused=True):
        nn.Module.__init__(self)
        self.bn_momentum = bn_momentum
        self.track_running_stats = track_running_stats
        self.dimension = dimension
        self.down_kernels, self.down_strides = downsample[0], downsample[1]
        self.fpn_scales_from_top = list(fpn_scales_from_top)
        self.roi_scales_from_top = list(roi_scales_from_top)
        self.residual_blocks = residual_blocks
        self.reps = reps
        self.fuse_adds, self.skip_unused = fuse_adds, skip_unused
        # storage type of the feature maps between the input layer and the maps handed to RPN / pooler:
        # torch.bfloat16 = BASELINE.json configs[4] (bf16 rows and weights, fp32 accumulation, fp32 statistics); in
        # training the rows' gradients are bf16 too, parameters, their gradients and the BatchNorm statistics fp32
        self.compute_dtype = torch.float32
        # storage type of the maps handed to RPN / pooler (SparseRCNN.head_dtype, set by the detector before each pass):
        # float32 = the backbone's maps widened (bf16 storage) or as they are; bfloat16 = bf16 rows, converted once from
        # an fp32 backbone or passed on as they are from a bf16 one
        self.head_dtype = torch.float32
        n_scales = len(nPlanesF)
        assert len(self.down_kernels) == n_scales - 1 == len(self.down_strides)
        in_channels = sum({'xyz': 3, 'color': 3, 'normal': 3}[e] for e in raw_elements)
        bn = dict(momentum=bn_momentum, track_running_stats=track_running_stats)

        self.layers_in_0 = scn.Sequential(scn.InputLayer(dimension, full_scale, mode=4))
        self.layers_in = scn.Sequential(
            scn.InputLayer(dimension, full_scale, mode=4),
            scn.SubmanifoldConvolution(dimension, in_channels, nPlanesF[0], 3, False))
        self.layers_out = scn.Sequential(scn.BatchNormReLU(nPlanesF[0], **bn), scn.OutputLayer(dimension))
        self.linear = nn.Linear(nPlanesF[0], 20)
        self.voxel_scale = voxel_scale
        self.rpn_map_sizes = np.array(rpn_map_sizes)
        self.rpn_3d_2d_selector = list(rpn_3d_2d_selector)
        self.convs_pro2d = nn.ModuleList(
            [scn.Convolution(dimension, nPlaneM, nPlaneM, [1, 1, int(z)], [1, 1, 1], False)
             for z in self.rpn_map_sizes[:, -1]])

        def block(m, a, b):
            if residual_blocks:
                assert a == b, "NetworkInNetwork branch is never taken by the detector configs"
                m.add(scn.ConcatTable()
                      .add(scn.Identity())
                      .add(scn.Sequential()
                           .add(scn.BatchNormLeakyReLU(a, leakiness=leakiness, **bn))
                           .add(scn.SubmanifoldConvolution(dimension, a, b, 3, False))
                           .add(scn.BatchNormLeakyReLU(b, leakiness=leakiness, **bn))
                           .add(scn.SubmanifoldConvolution(dimension, b, b, 3, False)))
                      ).add(scn.AddTable())
            else:
                m.add(scn.Sequential()
                      .add(scn.BatchNormLeakyReLU(a, leakiness=leakiness, **bn))
                      .add(scn.SubmanifoldConvolution(dimension, a, b, 3, False)))

        self.m_downs, self.m_shortcuts = nn.ModuleList(), nn.ModuleList()
        for k in range(n_scales):
            m = scn.Sequential()
            if k > 0:
                m.add(scn.Sequential()
                      .add(scn.BatchNormLeakyReLU(nPlanesF[k - 1], leakiness=leakiness, **bn))
                      .add(scn.Convolution(dimension, nPlanesF[k - 1], nPlanesF[k],
                                           self.down_kernels[k - 1], self.down_strides[k - 1], False)))
            for _ in range(reps):
                block(m, nPlanesF[k], nPlanesF[k])
            self.m_downs.append(m)
            self.m_shortcuts.append(scn.SubmanifoldConvolution(dimension, nPlanesF[k], nPlaneM, 1, False))

        self.m_ups, self.m_mergeds = nn.ModuleList(), nn.ModuleList()
        for k in range(n_scales - 1, 0, -1):
            self.m_ups.append(scn.Sequential()
                              .add(scn.BatchNormLeakyReLU(nPlaneM, leakiness=leakiness, **bn))
                              .add(scn.Deconvolution(dimension, nPlaneM, nPlaneM, self.down_kernels[k - 1],
                                                     self.down_strides[k - 1], False)))
            self.m_mergeds.append(scn.SubmanifoldConvolution(dimension, nPlaneM, nPlaneM, 3, False))

    # ------------------------------------------------------------------------------------
    def _to_compute(self, net):
        """input-layer output (fp32 [n, 9]) -> storage type of the backbone: bf16 rows are padded to 16 channels"""
        if self.compute_dtype == torch.float32 or net.features.dtype == self.compute_dtype:
            return net
        assert not torch.is_grad_enabled() or not net.features.requires_grad, \
            "bf16 storage: no gradient for the input features"
        f = net.features
        width = scn.SCN.stored_planes(f.shape[1], self.compute_dtype)
        if f.is_cuda and f.dtype == torch.float32 and self.compute_dtype == torch.bfloat16:
            net.features = scn.SCN.rows_to_bf16(f, width)       # (a pad and a cast took 1 ms of a 4 x 1 M-point step)
        else:
            net.features = torch.nn.functional.pad(f, (0, width - f.shape[1])).to(self.compute_dtype)
        return net

    def _from_compute(self, maps, converted=None):
        """maps -> the heads' storage type; `converted` (id -> tensor) shares the conversion of a map that both the RPN
        and the pooler consume"""
        if self.head_dtype == torch.bfloat16:
            converted = {} if converted is None else converted
            out = []
            for t in maps:
                if t is not None and t.features.dtype != torch.bfloat16:
                    if id(t) not in converted:
                        converted[id(t)] = scn.SparseConvNetTensor(_rows_to_bf16(t.features), t.metadata, t.spatial_size)
                    t = converted[id(t)]
                out.append(t)
            return out
        if self.compute_dtype == torch.float32:
            return maps
        return [None if t is None else scn.SparseConvNetTensor(t.features.float(), t.metadata, t.spatial_size) for t in maps]

    def forward(self, net0):
        if SIDE_STREAMS and _is_gpu_input(net0):
            return self._forward_async_geometry(net0)
        net1 = self.layers_in[1](self._to_compute(self.layers_in[0](net0)))
        return self.forward_fpn(net1)

    def _geometry_specs(self, size0):
        """The calls the library's geometry thread makes for the pyramid (d3d_geometry_async_start), as rows of 13 ints
        (kind, in_size, out_size, filter, stride): the d3d_conv_prepare calls in the order _geometry_steps makes them
        (kind 1 or 3, see below), the 3x3x3 submanifold rulebook (kind 0) of every level but the first right behind its
        grids and, after all grids, the lateral 1x1x1 rulebooks and the deconvolution views (kind 2) of the top-down
        path -- the views _geometry_steps builds with full=True.  For every level the rows it needs before its
        convolutions may be enqueued: (its last grid row, its 3x3x3 view row), -1 = none.
        -> (rows, rows per level, last row of all)"""
        n_scales = len(self.m_downs)
        n3d = len(self.fpn_scales_from_top)
        sel2d = sorted({i - n3d for i in self.rpn_3d_2d_selector if i >= n3d}) if self.skip_unused else range(n3d)
        pro2d = {n_scales - 1 - self.fpn_scales_from_top[i]: self.convs_pro2d[i] for i in sel2d}
        needed = max(self.fpn_scales_from_top + self.roi_scales_from_top) if self.skip_unused else n_scales - 1
        lowest_up = n_scales - 1 - min(n_scales - 1, needed)
        size = scn.toLongTensor(self.dimension, size0)
        three, one = [3] * self.dimension, [1] * self.dimension
        specs, last, later = [], [], []
        for k in range(n_scales):
            if k > 0:
                filt = scn.toLongTensor(self.dimension, self.down_kernels[k - 1])
                stride = scn.toLongTensor(self.dimension, self.down_strides[k - 1])
                out = (size - filt) // stride + 1
                # kind 3: no deconvolution / backward view of this rulebook will be asked for (inference, below the
                # finest level the top-down path reaches): its decoded table is not built
                need_dec = self.training or torch.is_grad_enabled() or k > lowest_up
                specs.append([1 if need_dec else 3] + size.tolist() + out.tolist() + filt.tolist() + stride.tolist())
                if k > lowest_up:
                    later.append([2] + out.tolist() + size.tolist() + filt.tolist() + stride.tolist())
                size = out
            if k in pro2d:
                conv = pro2d[k]
                out = (size - conv.filter_size) // conv.filter_stride + 1
                need_dec = self.training or torch.is_grad_enabled()
                specs.append([1 if need_dec else 3] + size.tolist() + out.tolist() + conv.filter_size.tolist()
                             + conv.filter_stride.tolist())
            grid_row = len(specs) - 1 if (k > 0 or k in pro2d) else -1     # the level's last grid / strided rulebook
            view_row = -1
            if k > 0:               # (level 0's is built by the caller while the point lists are sorted)
                specs.append([0] + size.tolist() + size.tolist() + three + one)
                view_row = len(specs) - 1
            if k >= lowest_up:
                later.append([0] + size.tolist() + size.tolist() + one + one)
            # a level waits for both: its 3x3x3 view starts as soon as the GRID exists, before the strided rulebook
            last.append((grid_row, view_row))
        specs += later
        return specs, last, len(specs) - 1

    def _forward_async_geometry(self, net0):
        """The pass of every GPU input, with the grid chain run by a thread of the library (d3d_geometry_async_start):
        every new grid costs a blocking read-back of its site count, and while this thread waited for one it could not
        enqueue the feature kernels of the level before -- by the end of the bottom-up path the caller's stream had
        caught up with its own launch thread.  Here the chain of all levels starts right after the input grid exists and
        runs at its own pace on the geometry stream; this thread picks a level up (count + stream dependency) when it is
        about to enqueue it.  A second thread of the library enqueues, on the plan stream, the rulebooks that are views
        of a finished grid (3x3x3 right behind each grid; lateral and deconvolution views at the end).  Same kernels on
        the same data as the one-stream pass (bit-identical).

        Both side streams start at `scene_start`, behind what the caller's stream held when the pass began, not behind
        what the pass enqueues there itself.  What the host enqueued on the caller's stream before the input grid's count
        read-back (the coordinates' copy, the grid) is complete when the hook below runs.  The torch tensors written on a
        side stream, and why each write follows the tensor's allocation and any fill (in deterministic mode torch fills
        every new tensor with NaN on the allocating stream):
          * the input layer's output features: allocated by resize_ on the caller's stream after the read-back, written
            on the plan stream by run_forward -- which makes the plan stream wait for the caller's stream first whenever
            that holds a fill of them or a copy of strided input features (SCN.InputLayer_updateOutput).  The only
            tensor allocated on the caller's stream and written on a side stream.
          * their bf16 rows (rows_to_bf16): allocated, filled and written on the plan stream, in that order.
        Everything else the side streams write -- grids, rulebooks, point lists, views -- lives in the metadata's arena,
        whose reuse from scene to scene is ordered by scene_start.  The caller's stream waits for the plan stream's input
        work (plan0) before it enqueues anything of the pass, so no block the allocator hands out again is still in use
        on a side stream; and for both side streams at the end."""
        main = torch.cuda.current_stream(net0[1].device)
        geo, pool, plan = _geometry_stream(main)
        scene_start, plan0 = pool
        scene_start.record(main)
        state = {}

        def after_input_build(md, size, run_forward):
            # The host has just seen the input grid's site count, i.e. the grid is complete: the side streams need not
            # wait for the caller's stream, which already holds the hash probes of level 0's rulebook (~0.1 ms).
            geo.wait_event(scene_start)
            md.set_geometry_stream(geo.cuda_stream)
            plan.wait_event(scene_start)
            with torch.cuda.stream(plan):
                scn.SCN.InputLayer_prepare(md)          # point lists: own scratch (no lane of the arena), ~0.1 ms
                means = run_forward(plan)               # ... and the per-voxel means right behind them, beside the
                                                        # sort of level 0's rulebook on the caller's stream
                if means is not None and self.compute_dtype == torch.bfloat16 and means.dtype == torch.float32:
                    # ... and their bf16 rows (one launch; a pad and a cast on the caller's stream were three and sat
                    # in front of the first convolution)
                    width = scn.SCN.stored_planes(means.shape[1], self.compute_dtype)
                    state["stored"] = (means, scn.SCN.rows_to_bf16(means, width))
                plan0.record(plan)
            # level 0's 3x3x3 rulebook on this stream (sort + transpose of the probed table, ~0.15 ms); the plan lane is
            # carved out of the feature lane only afterwards, and its stream continues behind this build (whose scratch
            # may reach into what becomes the plan lane)
            _tmark("input grid known (host)", -1, host=True)
            scn.SCN.SubmanifoldConvolution_prepare(size, (3,) * self.dimension, md)
            _tmark("level-0 rulebook", -1, main)
            _tmark("point lists + input means", -1, plan)
            plan.wait_stream(main)
            md.set_plan_stream(plan.cuda_stream)
            cache = getattr(self, "_spec_cache", None)
            key = tuple(scn.SCN._size3(size)) + (bool(self.training), torch.is_grad_enabled())
            if cache is None or cache[0] != key:
                cache = self._spec_cache = (key,) + self._geometry_specs(size)
            state["last"], state["all"] = cache[2], cache[3]
            # the chain of strided grids starts at once on the geometry stream (one read-back for all of its levels)
            md.geometry_async_start(cache[1], geo.cuda_stream, plan.cuda_stream)
            state["md"] = md
            main.wait_event(plan0)

        # (the neighbour table of level 0's 3x3x3 rulebook is probed while the input grid's site count is read back)
        scn.SCN.set_after_input_build(after_input_build, prefetch_filter=(3,) * self.dimension)
        try:
            net = self.layers_in[0](net0)                   # input layer: grid of level 0
        finally:
            scn.SCN.set_after_input_build(None)
        md = net.metadata
        n_scales = len(self.m_downs)
        try:
            def lane(k):
                _tmark("host enters", k, host=True)
                _tmark("main arrives", k, main)
                for idx in (state["all"],) if k >= n_scales else state["last"][k]:
                    if idx >= 0:
                        md.geometry_async_wait(idx, main.cuda_stream)
                _tmark("main continues", k, main)
                _tmark("host leaves", k, host=True)

            lane(0)
            stored = state.pop("stored", None)
            if stored is not None and stored[0] is net.features:
                net.features = stored[1]
            net = self.layers_in[1](self._to_compute(net))
            out = self.forward_fpn(net, prepared=True, lane=lane)
        finally:
            try:
                md.geometry_async_finish()
            finally:
                main.wait_stream(geo)
                main.wait_stream(plan)
                md.set_plan_stream(None)
                md.set_geometry_stream(None)
        return out

    def unused_modules(self):
        """Sub-modules whose parameters never receive a gradient under `skip_unused` (the reference computes some of them
        and discards the result, fpn_net.py:186-203; others -- layers_out, linear -- it only constructs): the top-down
        levels below the finest consumed map, their laterals and merges, unselected z-projections.  A data-parallel
        wrapper freezes them instead of searching the graph for them every step."""
        n_scales = len(self.m_downs)
        needed = max(self.fpn_scales_from_top + self.roi_scales_from_top) if self.skip_unused else n_scales - 1
        used_levels = min(n_scales - 1, needed)
        out = [self.layers_out, self.linear]
        out += [self.m_ups[k] for k in range(used_levels, len(self.m_ups))]
        consumed = set(self.fpn_scales_from_top) | set(self.roi_scales_from_top)
        # ups[k + 1] = m_mergeds[k](...) feeds heads only; the top-down path itself continues from the un-merged sum
        out += [self.m_mergeds[k] for k in range(len(self.m_mergeds))
                if k >= used_levels or (self.skip_unused and (k + 1) not in consumed)]
        out += [self.m_shortcuts[j] for j in range(0, n_scales - 1 - used_levels)]
        n3d = len(self.fpn_scales_from_top)
        sel2d = {i - n3d for i in self.rpn_3d_2d_selector if i >= n3d} if self.skip_unused else set(range(n3d))
        out += [self.convs_pro2d[i] for i in range(len(self.convs_pro2d)) if i not in sel2d]
        return out

    def _run_down(self, m, net):
        if not (self.fuse_adds and self.residual_blocks):
            return m(net)
        children = list(m._modules.values())
        i = 0
        while i < len(children):
            c = children[i]
            if isinstance(c, scn.ConcatTable):   # [Identity, (BN, conv, BN, conv)] followed by AddTable
                seq = c._modules['1']
                y = seq[0](net)
                y = seq[1](y)
                y = seq[2](y)
                net = seq[3](y, residual=net)     # out = conv(..) + identity branch
                i += 2
            else:
                net = c(net)
                i += 1
        return net

    def _geometry_steps(self, net, full):
        """Generator over the pyramid levels k = 0 .. n_scales-1: enqueues (on the current stream) everything level k
        needs -- the strided grid + rulebook k-1 -> k (one host read-back of the site count), the z-collapsing RPN
        projection grid of that level and, with `full`, the submanifold 3x3x3 / 1x1x1 rulebooks and the deconvolution
        view k -> k-1 (otherwise built by the first convolution that needs them) -- then yields k."""
        md, n_scales = net.metadata, len(self.m_downs)
        needed = max(self.fpn_scales_from_top + self.roi_scales_from_top) if self.skip_unused else n_scales - 1
        lowest_up = n_scales - 1 - min(n_scales - 1, needed)          # finest level the top-down path reaches
        n3d = len(self.fpn_scales_from_top)
        sel2d = sorted({i - n3d for i in self.rpn_3d_2d_selector if i >= n3d}) if self.skip_unused else range(n3d)
        pro2d = {n_scales - 1 - self.fpn_scales_from_top[i]: self.convs_pro2d[i] for i in sel2d}
        sizes = [net.spatial_size]
        for k in range(n_scales):
            if k > 0:
                filt = scn.toLongTensor(self.dimension, self.down_kernels[k - 1])
                stride = scn.toLongTensor(self.dimension, self.down_strides[k - 1])
                out = (sizes[-1] - filt) // stride + 1
                scn.SCN.Convolution_prepare(sizes[-1], out, filt, stride, md)
                sizes.append(out)
            size = sizes[k]
            if k in pro2d:
                conv = pro2d[k]
                scn.SCN.Convolution_prepare(size, (size - conv.filter_size) // conv.filter_stride + 1,
                                            conv.filter_size, conv.filter_stride, md)
            if full:
                scn.SCN.SubmanifoldConvolution_prepare(size, (3,) * self.dimension, md)
                if k >= lowest_up:                                                             # lateral 1x1x1
                    scn.SCN.SubmanifoldConvolution_prepare(size, (1,) * self.dimension, md)
                if k > lowest_up:
                    scn.SCN.Deconvolution_prepare(size, sizes[k - 1], self.down_kernels[k - 1], self.down_strides[k - 1],
                                                  md)
            yield k

    def prepare_geometry(self, net, full=False):
        """All strided grids / rulebooks of the pyramid, built before the first feature kernel: each new grid costs
        one host read-back of its site count, and here the stream holds only small geometry kernels when that
        happens, so the feature pass that follows is enqueued without a single synchronisation.
        full: also the submanifold and deconvolution rulebooks, which leaves the feature pass free of geometry kernels
        (serving.BuildingPipeline)."""
        for _ in self._geometry_steps(net, full):
            pass

    def stage_geometry(self, net0):
        """Stage 1 of 3 of a pipelined pass (serving.BuildingPipeline): input layer + every grid and rulebook."""
        net = self.layers_in[0](net0)
        self.prepare_geometry(net, full=True)
        return net

    def stage_features(self, net):
        """Stage 2: the feature pass over the prepared geometry (no host synchronisation)."""
        return self.forward_fpn(self.layers_in[1](self._to_compute(net)), prepared=True)

    def forward_fpn(self, net, prepared=False, lane=None):
        n_scales = len(self.m_downs)
        if not prepared:
            self.prepare_geometry(net)
        downs = []
        for k, m in enumerate(self.m_downs):
            if lane is not None:
                lane(k)
            net = self._run_down(m, net)
            downs.append(net)
        if lane is not None:
            lane(n_scales)
        _tmark("down path done")
        if (GROUP_CONVS and self.fuse_adds and not self.training and not torch.is_grad_enabled()
                and net.features.is_cuda and net.features.dtype == torch.float32):
            return self._top_down_grouped(net, downs)
        net = self.m_shortcuts[-1](net)
        ups = [net]
        needed = max(self.fpn_scales_from_top + self.roi_scales_from_top) if self.skip_unused else n_scales - 1
        consumed = set(self.fpn_scales_from_top) | set(self.roi_scales_from_top)
        for k in range(min(n_scales - 1, needed)):
            j = n_scales - 2 - k
            shortcut = self.m_shortcuts[j](downs[j])
            if self.fuse_adds:
                up = self.m_ups[k]
                net = up[1](up[0](net), residual=shortcut)
            else:
                net = scn.add_feature_planes([self.m_ups[k](net), shortcut])
            # a merged map that neither the RPN nor the pooler consumes is not computed (the reference computes and
            # drops it): the top-down path continues from `net`, the un-merged sum
            ups.append(self.m_mergeds[k](net) if (not self.skip_unused or (k + 1) in consumed) else None)
        _tmark("top-down done")
        rpn_maps_3d = [ups[i] for i in self.fpn_scales_from_top]
        selected_2d = {i - len(rpn_maps_3d) for i in self.rpn_3d_2d_selector if i >= len(rpn_maps_3d)}
        rpn_maps_2d = [self.convs_pro2d[i](rpn_maps_3d[i]) if (i in selected_2d or not self.skip_unused) else None
                       for i in range(len(rpn_maps_3d))]
        rpn_maps = rpn_maps_3d + rpn_maps_2d
        rpn_maps = [rpn_maps[i] for i in self.rpn_3d_2d_selector]
        roi_maps = [ups[i] for i in self.roi_scales_from_top]
        for i in range(len(rpn_maps_3d)):
            assert rpn_maps_3d[i].spatial_size.tolist() == [int(v) for v in self.rpn_map_sizes[i]]
        converted = {}
        return self._from_compute(rpn_maps, converted), self._from_compute(roi_maps, converted)

    def _top_down_grouped(self, net, downs):
        """The top-down path of forward_fpn with its independent convolutions grouped: one call for every needed
        shortcut, the dependent chain (statistics -> deconvolution with the level's shortcut as residual) with nothing in
        between, one call for the needed merged maps, one for the needed 2-D projections.  Returns what forward_fpn
        returns, bit for bit."""
        n_scales = len(self.m_downs)
        needed = max(self.fpn_scales_from_top + self.roi_scales_from_top) if self.skip_unused else n_scales - 1
        consumed = set(self.fpn_scales_from_top) | set(self.roi_scales_from_top)
        levels = min(n_scales - 1, needed)
        # the top shortcut feeds a BatchNorm (it keeps its column statistics), the others are residuals only
        laterals = scn.conv_group([(self.m_shortcuts[-1], net, None)]
                                  + [(self.m_shortcuts[n_scales - 2 - k], downs[n_scales - 2 - k], None)
                                     for k in range(levels)], want_stats=[True] + [False] * levels)
        net, laterals = laterals[0], laterals[1:]
        chain = [net]
        for k in range(levels):
            up = self.m_ups[k]
            net = up[1](up[0](net), residual=laterals[k])
            chain.append(net)
        merged = [k for k in range(levels) if not self.skip_unused or (k + 1) in consumed]
        outs = scn.conv_group([(self.m_mergeds[k], chain[k + 1], None) for k in merged], want_stats=False)
        ups = [chain[0]] + [None] * levels
        for k, t in zip(merged, outs):
            ups[k + 1] = t
        _tmark("top-down done")
        rpn_maps_3d = [ups[i] for i in self.fpn_scales_from_top]
        selected_2d = {i - len(rpn_maps_3d) for i in self.rpn_3d_2d_selector if i >= len(rpn_maps_3d)}
        pro = [i for i in range(len(rpn_maps_3d)) if (i in selected_2d or not self.skip_unused)]
        outs = scn.conv_group([(self.convs_pro2d[i], rpn_maps_3d[i], None) for i in pro], want_stats=False)
        rpn_maps_2d = [None] * len(rpn_maps_3d)
        for i, t in zip(pro, outs):
            rpn_maps_2d[i] = t
        rpn_maps = rpn_maps_3d + rpn_maps_2d
        rpn_maps = [rpn_maps[i] for i in self.rpn_3d_2d_selector]
        roi_maps = [ups[i] for i in self.roi_scales_from_top]
        for i in range(len(rpn_maps_3d)):
            assert rpn_maps_3d[i].spatial_size.tolist() == [int(v) for v in self.rpn_map_sizes[i]]
        converted = {}
        return self._from_compute(rpn_maps, converted), self._from_compute(roi_maps, converted)
