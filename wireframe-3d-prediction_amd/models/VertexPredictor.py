"""Drop-in `models.VertexPredictor.VertexPredictor` on the MI355X HIP path.

Keeps the reference's module tree (models/VertexPredictor.py:27-61) including the
LAZILY created `point_pool_proj` (reference :94-97): it is built
on the first forward with default nn.Linear init from the global RNG, exactly
when and how the reference does, so optimizer/state_dict behaviour is identical.
The `nn.Dropout` that closes each vertex_mlp stage (p = 0.0 by default, as in the reference) is
honoured in train() mode: its `p` is read on every call; while one is active the head runs on the
generic GEMM kernels, which draw the masks, whatever the batch size."""
import torch
import torch.nn as nn

from wf3d import dropout
from wf3d.functional import UnmaskedPoolFn, VertexFn, VertexParams


def _stage(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, n_out), nn.LayerNorm(n_out), nn.ReLU(inplace=True), nn.Dropout(0.0))


class VertexPredictor(nn.Module):
    def __init__(self, global_feature_dim=512, max_vertices=64, vertex_dim=4):
        super().__init__()
        self.max_vertices = max_vertices
        self.vertex_dim = vertex_dim
        self.vertex_mlp1 = _stage(global_feature_dim, 4096)
        self.vertex_mlp2 = _stage(4096, 2048)
        self.vertex_mlp3 = _stage(2048, 2048)
        self.vertex_mlp4 = _stage(2048, 1024)
        self.final_layer = nn.Linear(1024, max_vertices * vertex_dim)
        self.residual_proj1 = nn.Linear(global_feature_dim, 2048)
        self.residual_proj2 = nn.Linear(global_feature_dim, 1024)
        self.last_dropout_seed = None       # the seed the last train-mode call with an active site drew on the host
        self.last_dropout_seeds = None      # dropout_rng "device": the int32 [5] seed words of that call instead

    def ensure_point_pool_proj(self, in_features, device):
        """Create the lazy layer if absent (same moment/shape/init as the reference)."""
        if not hasattr(self, "point_pool_proj"):
            self.point_pool_proj = nn.Linear(in_features, self.residual_proj1.in_features).to(device)
        return self.point_pool_proj

    def _param_list(self, with_pool):
        m1, m2, m3, m4 = self.vertex_mlp1, self.vertex_mlp2, self.vertex_mlp3, self.vertex_mlp4
        fl, r1, r2 = self.final_layer, self.residual_proj1, self.residual_proj2
        return VertexParams(W1=m1[0].weight, b1=m1[0].bias, g1=m1[1].weight, be1=m1[1].bias,
                            W2=m2[0].weight, b2=m2[0].bias, g2=m2[1].weight, be2=m2[1].bias,
                            W3=m3[0].weight, b3=m3[0].bias, g3=m3[1].weight, be3=m3[1].bias,
                            W4=m4[0].weight, b4=m4[0].bias, g4=m4[1].weight, be4=m4[1].bias,
                            Wf=fl.weight, bf=fl.bias, Wr1=r1.weight, br1=r1.bias, Wr2=r2.weight, br2=r2.bias,
                            Wpp=self.point_pool_proj.weight if with_pool else None,
                            bpp=self.point_pool_proj.bias if with_pool else None)

    def _sites(self):
        # plain dict lookups (this runs on every forward): whatever module sits at index 3 of each stage now
        m = self._modules
        return (("vertex_mlp1.3", m["vertex_mlp1"]._modules["3"].p), ("vertex_mlp2.3", m["vertex_mlp2"]._modules["3"].p),
                ("vertex_mlp3.3", m["vertex_mlp3"]._modules["3"].p), ("vertex_mlp4.3", m["vertex_mlp4"]._modules["3"].p))

    def _dropout_ps(self):
        return dropout.site_ps(self, "vertex head", self._sites())

    def _dropout(self, device):
        return dropout.module_drop(self, "vertex head", self._sites(), device)

    def predict(self, global_features, upooled):
        """Vertex head from already-pooled point features, upooled = [mean | max] [B, 2C] (None -> no fusion)."""
        with_pool = upooled is not None
        if with_pool:
            self.ensure_point_pool_proj(upooled.shape[1], upooled.device)
        o, exist, counts = VertexFn.apply(global_features, upooled, self.max_vertices,
                                          self.vertex_dim, *self._param_list(with_pool),
                                          *self._dropout(global_features.device))
        return {"vertices": o,                            # non-contiguous [B, V, 3] view of the [B, V, 4] output (:122)
                "existence_probabilities": exist,
                "actual_vertex_counts": counts}

    def forward(self, global_features, point_features, target_vertex_counts=None):
        if point_features is not None:
            return self.predict(global_features, UnmaskedPoolFn.apply(point_features.float()))
        return self.predict(global_features, None)
