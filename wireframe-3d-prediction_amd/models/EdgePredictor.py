"""Drop-in `models.EdgePredictor.EdgePredictor` on the MI355X HIP path.

Module tree and state_dict keys follow reference models/EdgePredictor.py:31-68
(including `spatial_proj`, which the reference builds but never uses — kept for
RNG-order and state_dict compatibility).  forward() accepts a
padded batch [B, V, vertex_dim]; `forward_ragged` runs samples with different vertex
counts in one pass, which is how PointCloudToWireframe replaces the reference's
serial per-sample loop; `forward_padded` does the same with the counts in device memory
(capturable, any counts under one capture).  Under torch.no_grad() with no dropout active,
wf3d.config.set_edge_inference("stream") sends all three to the forward-only path (wf3d.infer.edge_stream), which
`forward_stream` calls directly."""
import torch
import torch.nn as nn

from wf3d import config, dropout, infer, ops
from wf3d.functional import EdgeFn, EdgeParams, edge_index_lists


class EdgePredictor(nn.Module):
    def __init__(self, vertex_dim=3, hidden_dim=512, num_heads=8):
        super().__init__()
        if not 1 <= vertex_dim <= 8:
            raise ValueError("the HIP edge head takes 1..8 coordinates per vertex (reference default: 3)")
        if hidden_dim % 16 or hidden_dim % num_heads or (hidden_dim // num_heads) % 4:
            # said at construction, not by a kernel in the middle of a backward pass: the row kernels work on 16-byte
            # pieces of the hidden_dim / 4-wide layer, the attention kernels on 4-column pieces of a head.  Head widths 64
            # to 128 run on the matrix cores at any vertex count; widths up to 60 and above 128 on the VALU kernels, which
            # above 128 refuse a call whose staged rows do not fit the LDS (about 140 vertices at width 132)
            raise ValueError(f"the HIP edge head needs hidden_dim % 16 == 0 and a head width (hidden_dim / num_heads) % 4 == 0 "
                             f"(got hidden_dim={hidden_dim}, num_heads={num_heads})")
        h = hidden_dim
        self.vertex_proj = nn.Sequential(
            nn.Linear(vertex_dim, h // 2), nn.LayerNorm(h // 2), nn.GELU(),
            nn.Linear(h // 2, h), nn.LayerNorm(h), nn.Dropout(0.1))
        self.attention = nn.MultiheadAttention(embed_dim=h, num_heads=num_heads, dropout=0.1, batch_first=True)
        self.spatial_proj = nn.Sequential(nn.Linear(vertex_dim, h // 4), nn.GELU(), nn.Linear(h // 4, h // 4))
        self.edge_mlp = nn.Sequential(
            nn.Linear(2 * h + 2 * vertex_dim + 1, h), nn.LayerNorm(h), nn.GELU(), nn.Dropout(0.1),
            nn.Linear(h, h // 2), nn.LayerNorm(h // 2), nn.GELU(), nn.Dropout(0.1),
            nn.Linear(h // 2, h // 4), nn.GELU(),
            nn.Linear(h // 4, 1))
        self._heads = num_heads
        self.last_dropout_seed = None       # the seed the last train-mode call with an active site drew on the host
        self.last_dropout_seeds = None      # dropout_rng "device": the int32 [5] seed words of that call instead

    def _get_edge_indices(self, num_vertices):
        """[E, 2] int64, all i<j in lexicographic order (reference :70-89)."""
        dev = next(self.parameters()).device
        if num_vertices < 2:
            return torch.tensor([], dtype=torch.long, device=dev)      # 1-D empty, as the reference yields
        return torch.triu_indices(num_vertices, num_vertices, 1, device=dev).t().contiguous()

    def _param_list(self):
        vp, at, em = self.vertex_proj, self.attention, self.edge_mlp
        return EdgeParams(P0w=vp[0].weight, P0b=vp[0].bias, P1g=vp[1].weight, P1b=vp[1].bias,
                          P3w=vp[3].weight, P3b=vp[3].bias, P4g=vp[4].weight, P4b=vp[4].bias,
                          Aw=at.in_proj_weight, Ab=at.in_proj_bias, Ow=at.out_proj.weight, Ob=at.out_proj.bias,
                          M0w=em[0].weight, M0b=em[0].bias, M1g=em[1].weight, M1b=em[1].bias,
                          M4w=em[4].weight, M4b=em[4].bias, M5g=em[5].weight, M5b=em[5].bias,
                          M8w=em[8].weight, M8b=em[8].bias, M10w=em[10].weight, M10b=em[10].bias)

    def _sites(self):
        # plain dict lookups (this runs on every forward): whatever module sits at the index now
        m = self._modules
        vp, em = m["vertex_proj"]._modules, m["edge_mlp"]._modules
        return (("vertex_proj.5", vp["5"].p), ("attention", m["attention"].dropout),
                ("edge_mlp.3", em["3"].p), ("edge_mlp.7", em["7"].p))

    def _dropout_ps(self):
        return dropout.site_ps(self, "edge head", self._sites())

    def _dropout(self, device):
        return dropout.module_drop(self, "edge head", self._sites(), device)

    @staticmethod
    def _ragged_counts(vertices, counts, who):
        if len(counts) != vertices.shape[0]:
            raise ValueError(f"{who}: {len(counts)} counts for a batch of {vertices.shape[0]}")
        counts = [min(int(c), vertices.shape[1]) for c in counts]      # `vertices[i, :count]` cannot take more than there is
        if any(c < 2 for c in counts):
            # the reference indexes a 1-D empty index tensor here (EdgePredictor.py:118)
            raise IndexError("too many indices for tensor of dimension 1")
        return counts

    @staticmethod
    def _padded_meta(vertices, counts, tail, who):
        if tail not in ("compute", "skip"):
            raise ValueError(f"{who}: tail must be 'compute' or 'skip'")
        B, V, _ = vertices.shape
        if not torch.is_tensor(counts) or counts.dim() != 1 or counts.shape[0] != B:
            raise ValueError(f"{who}: counts must be a 1-D tensor of {B} counts")
        if counts.dtype.is_floating_point or counts.dtype.is_complex:
            raise ValueError(f"{who}: counts must be integers")
        return ops.EdgeMeta.device(counts.to(device=vertices.device, dtype=torch.int64).contiguous(), B, V, tail=tail)

    def forward_ragged(self, vertices, counts):
        """vertices [B, Vmax, 3]; sample s uses its first counts[s] vertices.
        Returns zero-padded probabilities [B, max_s E_s]."""
        counts = self._ragged_counts(vertices, counts, "forward_ragged")
        if self._stream():
            return self._edge_stream(vertices, ops.EdgeMeta.get(counts, vertices.device))
        return EdgeFn.apply(vertices.float(), tuple(counts), self._heads, config.precision(), *self._param_list(),
                            *self._dropout(vertices.device))

    def _stream(self):
        """The forward-only path (wf3d.infer.edge_stream) serves this call: the edge setting asks for it, grad mode is
        off and no dropout probability is active (the block kernels draw no masks)."""
        return config.edge_inference() == "stream" and not torch.is_grad_enabled() and not any(self._dropout_ps())

    def _edge_stream(self, vertices, meta, rows=None):
        return infer.edge_stream(vertices.float(), meta, self._heads, config.precision(), self._param_list(), rows)

    def forward_stream(self, vertices, counts, rows=None, tail="compute"):
        """The forward-only edge head called directly, whatever the setting: edge_probs as forward_ragged (counts: a
        list of host ints) or forward_padded (counts: an integer tensor [B] on the device, never read on the host; `tail`
        as there) return them, with the edge rows walked in blocks of `rows` (default config.INFER_EDGE_ROWS, a
        multiple of 8) and no activation kept.  No autograd graph is recorded.  It has no dropout: ValueError while a
        dropout probability is active (train mode with p > 0)."""
        if any(self._dropout_ps()):
            raise ValueError("EdgePredictor.forward_stream: the forward-only path has no dropout; call eval() or set every "
                             "dropout probability of the edge head to 0")
        if torch.is_tensor(counts):
            return self._edge_stream(vertices, self._padded_meta(vertices, counts, tail, "forward_stream"), rows)
        return self._edge_stream(vertices, ops.EdgeMeta.get(self._ragged_counts(vertices, counts, "forward_stream"),
                                                            vertices.device), rows)

    def forward_padded(self, vertices, counts, return_layout=False, tail="compute"):
        """vertices [B, V, 3]; counts: integer tensor [B] on the device, never read on the host.  Sample s uses its
        first c_s vertices, c_s clamped like `vertices[s, :counts[s]]` slicing.  Returns [B, V(V-1)/2]: sample s's first
        c_s(c_s-1)/2 entries in the reference's pair order, exactly 0.0 after, so that out[:, :max_s E_s] is what
        forward_ragged returns.  The row layout is built on the device in this call (capturable); the edge rows run at
        their worst case, counts = V.  A sample with fewer than 2 vertices gets an all-zero row (forward_ragged raises
        the reference's IndexError; that would need a host read here).
        return_layout=True: also return the clamped counts (int64 [B]) and the edge width max_s E_s (0-d int64).
        tail="skip": the edge-row launches read the live pair total from device memory when they run and stop at the
        256-row boundary above it instead of running all B*V(V-1)/2 rows; the output and every gradient are bit-identical
        to tail="compute".  It applies where the edge MLP runs on the split route (precision "bf16x3" / "bf16", enough
        rows, a row total B*V(V-1)/2 that is a multiple of 8, a logits layer the row-dot kernel takes, as the default
        hidden_dim = 512); elsewhere the tail is computed."""
        meta = self._padded_meta(vertices, counts, tail, "forward_padded")
        if self._stream():
            probs = self._edge_stream(vertices, meta)
        else:
            probs = EdgeFn.apply(vertices.float(), meta, self._heads, config.precision(), *self._param_list(),
                                 *self._dropout(vertices.device))
        return (probs, meta.counts, meta.width) if return_layout else probs

    def forward(self, vertices):
        b, v, _ = vertices.shape
        probs = self.forward_ragged(vertices, [v] * b)
        return probs, edge_index_lists([v])[0]
