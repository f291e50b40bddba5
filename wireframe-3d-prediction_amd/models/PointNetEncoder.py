"""Drop-in `models.PointNetEncoder.PointNetEncoder` on the MI355X HIP path.

Same constructor, attribute names and state_dict keys as the reference class
(reference models/PointNetEncoder.py:19-65: `mlp` Sequential with parameters at
indices 0,1,4,5,...,4n and `feature_fusion` at 0,1,3,4,6).  The nn modules here
are parameter containers only: forward never calls them, it hands their tensors
to wf3d.functional.EncoderFn (HIP kernels through the C ABI).  The `nn.Dropout` after each
Linear, LayerNorm, ReLU block of `mlp` (p = 0.0 by default, as in the reference) is honoured in
train() mode: its `p` is read on every call and the kernels draw the masks."""
import torch
import torch.nn as nn

from wf3d import config, dropout, infer, ops
from wf3d.functional import EncoderFn, EncoderFnPacked, EncoderFnPackedSkip, FusionFn, FusionParams


def _point_block(n_in, n_out):
    return [nn.Linear(n_in, n_out), nn.LayerNorm(n_out), nn.ReLU(inplace=True), nn.Dropout(0.0)]


class PointNetEncoder(nn.Module):
    def __init__(self, input_dim=8, hidden_dims=[512, 1024, 2048, 1024], output_dim=512):
        super().__init__()
        bad = [h for h in hidden_dims if h % 4 or not 0 < h <= 4096]
        if bad or output_dim % 2 or output_dim <= 0:
            # said here, not by a kernel in the middle of a backward pass: LayerNorm rows are handled in 16-byte pieces
            # (hidden widths, and the fusion MLP's 4 x / 2 x output_dim) and kept in registers up to 4096 columns
            raise ValueError(f"the HIP encoder needs hidden widths that are multiples of 4 (<= 4096) and an even output_dim "
                             f"(got hidden_dims={list(hidden_dims)}, output_dim={output_dim})")
        widths = [input_dim] + list(hidden_dims)
        stack = []
        for n_in, n_out in zip(widths[:-1], widths[1:]):
            stack += _point_block(n_in, n_out)
        stack.append(nn.Linear(widths[-1], output_dim))
        self.mlp = nn.Sequential(*stack)
        # declared (parameter-free) by the reference, never used in its forward
        self.global_max_pool = nn.AdaptiveMaxPool1d(1)
        self.global_avg_pool = nn.AdaptiveAvgPool1d(1)
        d = output_dim
        self.feature_fusion = nn.Sequential(
            nn.Linear(2 * d, 4 * d), nn.LayerNorm(4 * d), nn.ReLU(inplace=True),
            nn.Linear(4 * d, 2 * d), nn.LayerNorm(2 * d), nn.ReLU(inplace=True),
            nn.Linear(2 * d, d))
        self._n_hidden = len(hidden_dims)
        self._site_keys = tuple(str(4 * i + 3) for i in range(len(hidden_dims)))      # mlp's nn.Dropout modules
        self.precision = None          # None -> wf3d.config.precision() ("bf16x3" | "bf16" | "fp32")
        self._packed_tail = "compute"  # set_packed_tail
        self.last_dropout_seed = None       # the seed the last train-mode call with an active site drew on the host
        self.last_dropout_seeds = None      # dropout_rng "device": the int32 [5] seed words of that call instead

    def _mlp_params(self):
        ps = []
        for i in range(self._n_hidden):
            lin, ln = self.mlp[4 * i], self.mlp[4 * i + 1]
            ps += [lin.weight, lin.bias, ln.weight, ln.bias]
        last = self.mlp[4 * self._n_hidden]
        return ps + [last.weight, last.bias]

    def _fusion_params(self):
        ff = self.feature_fusion
        return FusionParams(F0w=ff[0].weight, F0b=ff[0].bias, F1g=ff[1].weight, F1b=ff[1].bias,
                            F3w=ff[3].weight, F3b=ff[3].bias, F4g=ff[4].weight, F4b=ff[4].bias,
                            F6w=ff[6].weight, F6b=ff[6].bias)

    def _sites(self):
        # plain dict lookups (this runs on every forward; Sequential.__getitem__ walks its modules): whatever module sits
        # at the index now, a replaced nn.Dropout included
        mods = self._modules["mlp"]._modules
        return tuple([("mlp." + k, mods[k].p) for k in self._site_keys])

    def _dropout_ps(self):
        return dropout.site_ps(self, "encoder", self._sites())

    def _dropout(self, device):
        return dropout.module_drop(self, "encoder", self._sites(), device)

    def _stream_ok(self):
        """The forward-only path draws no masks: it serves a call only while no dropout site is active."""
        return not any(self._dropout_ps())

    def encode(self, x):
        """(global, point_features, unmasked_pooled [B, 2C] = [mean | max]): the extra pools are what
        VertexPredictor would recompute from point_features (VertexPredictor.py:86-88)."""
        if x.dim() != 3:
            raise ValueError(f"expected (batch, num_points, input_dim), got {tuple(x.shape)}")
        pooled, pf, upooled = EncoderFn.apply(x.float(), self._n_hidden, self.precision or config.precision(),
                                              *self._mlp_params(), *self._dropout(x.device))
        g = FusionFn.apply(pooled, *self._fusion_params())
        return g, pf, upooled

    def set_packed_tail(self, tail):
        """What encode_packed does with the rows of a capacity batch behind its clouds: "compute" (default) runs the
        per-point MLP over all `capacity` rows; "skip" stops it at the live row total (encode_packed).  A setting of
        the module, like PointCloudToWireframe.set_edge_layout's tail, so that encode_packed / forward_packed keep
        their signatures.  Returns self."""
        if tail not in ("compute", "skip"):
            raise ValueError(f"tail must be 'compute' or 'skip' (got {tail!r})")
        self._packed_tail = tail
        return self

    def _check_tail(self, capacity):
        """The packed tail mode of this call, checked on the host before any device work."""
        tail = getattr(self, "_packed_tail", "compute")
        if tail == "skip" and capacity is None:
            raise ValueError("the packed tail mode 'skip' needs a capacity: without one there are no rows to skip "
                             "(pass capacity=, or set_packed_tail('compute'))")
        return tail

    def encode_packed(self, points, point_counts, capacity=None):
        """encode() of a packed batch (wf3d.packed.pack): points [M, input_dim] = the clouds concatenated along the point
        axis, point_counts their lengths (host values: a list or a CPU int tensor).  Returns (global [B, C],
        point_features [M, C], unmasked_pooled [B, 2C]); cloud b's are those of encode(x_b[None]).  Nothing is read back
        from the device; the row layout of a list of counts is built once and cached (ops.PackedLayout.get).

        capacity (a multiple of ops.ROW_PAD): points is [capacity, input_dim], the clouds in its first rows and anything
        finite behind them, point_features is [capacity, C], and every launch shape depends on (B, capacity) alone.
        point_counts may then also be a CUDA int64 / int32 tensor [B]: it is never read on the host, the row layout is
        built on the device inside this call (ops.DevicePackedLayout; counts it has to clamp are flagged in its status
        word, which forward_packed returns), so one graph capture serves any counts.

        set_packed_tail (the mode of calls with a capacity): "compute" (default) runs the per-point MLP over all `capacity`
        rows; "skip" stops it, forward and backward, at R256 = the live row total rounded up to 256 rows (at most capacity), read on the device
        by each launch, so one capture still serves any counts.  Under "skip"
          - rows >= R256 of points are not read: they may hold anything, where "compute" needs them finite;
          - rows >= R256 of the returned point_features are unspecified;
          - rows >= R256 of a gradient arriving for point_features are not read;
        and every other output and every gradient equals the "compute" mode bit for bit: the skipped rows are pad rows, whose
        backward is exact zeros.  The mode needs the split routes (bf16x3 / bf16 precision, capacity >=
        config.SPLIT_MIN_ROWS, the fused first layer, hidden widths the split kernels take: the default ones do); any
        other configuration computes the tail as "compute" does (functional._encoder_live).  "skip" without a capacity
        raises ValueError."""
        return self._encode_packed(points, point_counts, capacity)[:3]

    def _encode_packed(self, points, point_counts, capacity):
        """encode_packed, and the layout it ran on."""
        tail = self._check_tail(capacity)
        layout = self._packed_layout(points, point_counts, capacity)
        fn = EncoderFnPackedSkip if tail == "skip" else EncoderFnPacked
        pooled, pf, upooled = fn.apply(points.float(), layout, self._n_hidden, self.precision or config.precision(),
                                       *self._mlp_params(), *self._dropout(points.device))
        g = FusionFn.apply(pooled, *self._fusion_params())
        return g, pf, upooled, layout

    def _packed_layout(self, points, point_counts, capacity):
        """The arguments of a packed call checked on the host, and the row layout of its counts."""
        on_device = capacity is not None and torch.is_tensor(point_counts) and point_counts.is_cuda
        counts = None if on_device else ops.point_counts_list(point_counts)
        if not torch.is_tensor(points) or points.dim() != 2:
            raise ValueError("expected packed points (sum of point counts, input_dim)")
        if capacity is not None:
            if points.shape[0] != ops.check_capacity(capacity):
                raise ValueError(f"with capacity={capacity} the packed points must have {capacity} rows (got {points.shape[0]})")
        elif sum(counts) != points.shape[0]:
            raise ValueError(f"point counts sum to {sum(counts)}, but there are {points.shape[0]} packed points")
        if not points.is_cuda:
            raise RuntimeError("wf3d: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
        if not points.is_contiguous():
            raise ValueError("packed points must be contiguous")
        if points.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("wf3d: a packed batch that requires grad is not supported (detach the points)")
        if on_device:
            if point_counts.dim() != 1 or point_counts.shape[0] < 1 or point_counts.dtype not in (torch.int64, torch.int32):
                raise ValueError("device point counts must be a 1-D int64 or int32 tensor of at least one cloud")
            if point_counts.device != points.device:
                raise ValueError("device point counts must be on the points' device")
            return ops.DevicePackedLayout(point_counts.shape[0], capacity, points.device).build(point_counts.contiguous())
        return ops.PackedLayout.get(counts, points.device, capacity)

    def encode_stream(self, x, want_pf=False, rows=None):
        """encode() on the forward-only path (wf3d.infer): the per-point MLP walks the B * N rows in blocks of `rows`
        (a positive multiple of 8; None: wf3d.config.INFER_ROWS), keeps nothing for a backward and pools the blocks as
        they pass.  Returns (global, point_features [B, N, C] if want_pf else None, unmasked_pooled); runs under
        torch.no_grad() whatever the caller's grad mode.  It has no dropout: ValueError while a site of `mlp` is active
        (train mode with p > 0)."""
        self._check_stream("encode_stream")
        if x.dim() != 3:
            raise ValueError(f"expected (batch, num_points, input_dim), got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("wf3d: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
        B, N, Din = x.shape
        with torch.no_grad():
            x2 = x.float().reshape(B * N, Din).contiguous()
            po, pf = infer.encoder_stream(x2, infer.DenseRows(B, N, x.device), self._n_hidden,
                                          self.precision or config.precision(), self._mlp_params(), rows, want_pf)
            g = FusionFn.apply(po.masked, *self._fusion_params())
        return g, (pf.view(B, N, -1) if want_pf else None), po.unmasked

    def encode_packed_stream(self, points, point_counts, capacity=None, want_pf=False, rows=None):
        """encode_packed() on the forward-only path (encode_stream).  With host counts the blocks stop at the live row
        total rounded up to 8 (rows of a requested point_features behind that are zeros); with device counts and a
        capacity all `capacity` rows are walked, the pools ignore the rows behind the clouds, and nothing is read on the
        host.  The packed tail mode does not apply: there is no backward whose rows could be skipped."""
        return self._encode_packed_stream(points, point_counts, capacity, want_pf, rows)[:3]

    def _check_stream(self, who):
        if not self._stream_ok():
            raise ValueError(f"PointNetEncoder.{who}: the forward-only path has no dropout; call eval() or set every "
                             "dropout probability of the encoder to 0")

    def _encode_packed_stream(self, points, point_counts, capacity, want_pf=False, rows=None):
        """encode_packed_stream, and the layout it ran on."""
        self._check_stream("encode_packed_stream")
        layout = self._packed_layout(points, point_counts, capacity)
        walk = points.shape[0] if layout.M is None else min(points.shape[0], -(-layout.M // 8) * 8)
        with torch.no_grad():
            po, pf = infer.encoder_stream(points.float(), layout, self._n_hidden, self.precision or config.precision(),
                                          self._mlp_params(), rows, want_pf, walk=walk)
            g = FusionFn.apply(po.masked, *self._fusion_params())
        return g, pf, po.unmasked, layout

    def forward(self, x):
        if config.inference() == "stream" and not torch.is_grad_enabled() and self._stream_ok():
            return self.encode_stream(x, want_pf=True)[:2]
        g, pf, _ = self.encode(x)
        return g, pf
