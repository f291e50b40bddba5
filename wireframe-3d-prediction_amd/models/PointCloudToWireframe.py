"""Drop-in `models.PointCloudToWireframe.PointCloudToWireframe` (reference
models/PointCloudToWireframe.py:10-121) on the MI355X HIP path.

Differences in HOW, not WHAT: point_features is pooled once for both heads, and
the edge head runs all samples of the batch in one ragged pass instead of a
Python loop of batch-1 calls with a device->host sync each.  Outputs (keys,
shapes, dtypes, zero padding, edge_indices list-of-lists) are the reference's."""
import torch
import torch.nn as nn

from models.EdgePredictor import EdgePredictor
from models.PointNetEncoder import PointNetEncoder
from models.VertexPredictor import VertexPredictor
from wf3d import config
from wf3d.functional import EdgeIndexLists, edge_index_lists


class PointCloudToWireframe(nn.Module):
    def __init__(self, input_dim=8, max_vertices=64):
        super().__init__()
        self.max_vertices = max_vertices
        self.encoder = PointNetEncoder(input_dim=input_dim)
        self.vertex_predictor = VertexPredictor(global_feature_dim=512, max_vertices=max_vertices)
        self.edge_predictor = EdgePredictor(vertex_dim=3)
        self._count_cache = (None, -1, None)         # (the tensor object itself, its _version, host ints)
        self._edge_layout = "ragged"                 # set_edge_layout
        self._edge_tail = "compute"

    def set_dropout(self, p):
        """Set every dropout probability of the edge head (the only non-zero ones by default)."""
        ep = self.edge_predictor
        ep.vertex_proj[5].p = ep.edge_mlp[3].p = ep.edge_mlp[7].p = float(p)
        ep.attention.dropout = float(p)
        return self

    def set_encoder_dropout(self, p):
        """Set the dropout probability behind every Linear, LayerNorm, ReLU block of the encoder's per-point MLP
        (encoder.mlp[3], [7], ...; 0.0 by default).  Returns self."""
        for m in self.encoder.mlp:
            if isinstance(m, nn.Dropout):
                m.p = float(p)
        return self

    def set_vertex_dropout(self, p):
        """Set the dropout probability that closes each of the vertex head's four stages (vertex_mlp{1..4}[3]; 0.0 by
        default).  Returns self."""
        vp = self.vertex_predictor
        for st in (vp.vertex_mlp1, vp.vertex_mlp2, vp.vertex_mlp3, vp.vertex_mlp4):
            st[3].p = float(p)
        return self

    def _host_counts(self, t, slot="_count_cache"):
        """Vertex counts as Python ints.  One device->host read per call (the reference does one
        `.item()` per sample, :80/:90).  The read is skipped only when the SAME tensor object is
        passed again unmodified, as train.py does every step (train.py:127): the cache holds a
        reference to that tensor — so its storage cannot be freed and handed to another batch's
        counts — and compares identity plus the autograd version counter, which every in-place
        torch op bumps.  (Writes that bypass the counter — `.data`, raw pointers — are not seen;
        pass a CPU tensor or a fresh tensor then.)  CPU tensors are read directly, no sync."""
        if not t.is_cuda:
            return [int(c) for c in t.tolist()]
        ref, ver, vals = getattr(self, slot, (None, -1, None))
        if ref is t and ver == t._version:
            return vals
        vals = [int(c) for c in t.tolist()]
        setattr(self, slot, (t, t._version, vals))
        return vals

    def set_edge_layout(self, layout, tail=None):
        """"ragged" (default): the edge head's row layout is built from the counts read on the host — the output is the
        reference's exactly.  "padded": the counts stay on the device (target counts in train mode, actual_vertex_counts
        otherwise) and the layout is built there, so that a forward (and a training step) can be captured once and
        replayed on batches with any counts.  Then `edge_probs` is [B, V(V-1)/2] (zeros past each sample's pairs; its
        first `edge_width` columns are the ragged output), `edge_indices` is a read-only sequence that reads the counts
        on first access, and two keys are added: `edge_counts` (int64 [B], the clamped counts used) and `edge_width`
        (0-d int64 tensor, max_s E_s).  A sample with fewer than 2 vertices gets an all-zero row instead of the
        reference's IndexError.
        tail (padded only): "compute" (default) runs every edge-row launch over all B*V(V-1)/2 rows; "skip" lets them
        stop at the live pair total, read from device memory by the kernels (EdgePredictor.forward_padded): same
        outputs and gradients bit for bit, less work when the counts are below max_vertices."""
        if layout not in ("ragged", "padded"):
            raise ValueError("edge layout must be 'ragged' or 'padded'")
        if tail is not None and layout != "padded":
            raise ValueError("tail applies to the 'padded' edge layout only")
        if tail not in (None, "compute", "skip"):
            raise ValueError("edge tail must be 'compute' or 'skip'")
        self._edge_layout = layout
        self._edge_tail = tail or "compute"
        return self

    def _forward_padded(self, g, vo, target_vertex_counts):
        verts = vo["vertices"]
        b = verts.shape[0]
        if self.training and target_vertex_counts is not None:
            tc = torch.as_tensor(target_vertex_counts)
            if tc.dim() != 1 or tc.shape[0] < b:
                n = tc.shape[0] if tc.dim() else 0
                raise IndexError(f"index {n} is out of bounds for dimension 0 with size {n}")
            counts = tc[:b]
        else:
            counts = vo["actual_vertex_counts"]
        probs, ecounts, width = self.edge_predictor.forward_padded(verts, counts, return_layout=True,
                                                                     tail=getattr(self, "_edge_tail", "compute"))
        return {"vertices": verts,
                "existence_probabilities": vo["existence_probabilities"],
                "edge_probs": probs,
                "edge_indices": EdgeIndexLists(ecounts),
                "global_features": g,
                "actual_vertex_counts": vo["actual_vertex_counts"],
                "edge_counts": ecounts,
                "edge_width": width}

    def _stream(self):
        """The encoder stage takes the forward-only path (wf3d.infer): the setting asks for it, grad mode is off and no
        dropout site of the encoder is active (the block walk draws no masks; EdgePredictor._stream's rule).  Without
        an active site train() / eval() does not enter the decision."""
        return config.inference() == "stream" and not torch.is_grad_enabled() and self.encoder._stream_ok()

    def forward(self, point_cloud, target_vertex_counts=None):
        if self._stream():
            g, _pf, upooled = self.encoder.encode_stream(point_cloud)
        else:
            g, _pf, upooled = self.encoder.encode(point_cloud)
        return self._heads(g, upooled, target_vertex_counts)

    def set_packed_tail(self, tail):
        """The encoder's tail mode for packed batches with a capacity: "compute" (default) or "skip"
        (PointNetEncoder.set_packed_tail; forward_packed says what changes).  Returns self."""
        self.encoder.set_packed_tail(tail)
        return self

    def forward_packed(self, points, point_counts, target_vertex_counts=None, capacity=None):
        """forward() of a packed batch: points [M, input_dim] = clouds of any lengths concatenated along the point axis
        (wf3d.packed.pack), point_counts their lengths — host values, a list or a CPU int tensor; a CUDA tensor is read
        once, as target_vertex_counts is.  Same output dict as forward(); sample b's entries are those of
        forward(x_b[None]) on that cloud alone (not those of the zero-padded batch: the vertex head's pools count pad rows).

        capacity (a multiple of 256): points is [capacity, input_dim] with the clouds in its first rows
        (wf3d.packed.pack_into fills such a buffer), and every launch of the encoder depends on (B, capacity) alone.  A
        CUDA int64 / int32 point_counts [B] is then never read on the host: the row layout is built on the device in this
        call, and the dict gains `point_status` (int32 [1] on the device: bit 0 = counts were clamped to the capacity,
        bit 1 = some cloud has no rows; such a cloud pools to zeros and passes no gradient).  With the "padded" edge
        layout one captured step then serves batches of any point counts.

        set_packed_tail("skip") (with a capacity) stops the encoder's per-point MLP at the live row total rounded up to
        256 rows instead of computing all `capacity` rows (PointNetEncoder.encode_packed): the rows of `points` behind
        that are not read and may hold anything, every output and gradient equals the "compute" mode bit for bit; without
        a capacity the call raises ValueError.  It composes with set_edge_layout("padded", tail="skip"), which does the
        same for the edge rows."""
        self.encoder._check_tail(capacity)
        if capacity is None and torch.is_tensor(point_counts) and point_counts.is_cuda:
            point_counts = self._host_counts(point_counts, "_point_count_cache")
        if self._stream():
            g, _pf, upooled, layout = self.encoder._encode_packed_stream(points, point_counts, capacity)
        else:
            g, _pf, upooled, layout = self.encoder._encode_packed(points, point_counts, capacity)
        out = self._heads(g, upooled, target_vertex_counts)
        if layout.status is not None:
            out["point_status"] = layout.status
        return out

    def _heads(self, g, upooled, target_vertex_counts):
        vo = self.vertex_predictor.predict(g, upooled)
        if getattr(self, "_edge_layout", "ragged") == "padded":
            return self._forward_padded(g, vo, target_vertex_counts)
        verts = vo["vertices"]
        if self.training and target_vertex_counts is not None:
            counts = self._host_counts(target_vertex_counts)          # ground-truth counts (:77-86)
        else:
            counts = [int(c) for c in vo["actual_vertex_counts"].tolist()]   # data-dependent (:87-97)
        b = verts.shape[0]
        if len(counts) < b:
            # the reference reads target_vertex_counts[i] for every sample i of the batch (:78-80)
            raise IndexError(f"index {len(counts)} is out of bounds for dimension 0 with size {len(counts)}")
        counts = counts[:b]                                                   # entries beyond the batch are never read there
        v = self.max_vertices
        counts = [min(c, v) if c >= 0 else max(v + c, 0) for c in counts]    # what `[:count]` slicing does
        probs = self.edge_predictor.forward_ragged(verts, counts)
        return {"vertices": verts,
                "existence_probabilities": vo["existence_probabilities"],
                "edge_probs": probs,
                "edge_indices": edge_index_lists(counts),
                "global_features": g,
                "actual_vertex_counts": vo["actual_vertex_counts"]}
