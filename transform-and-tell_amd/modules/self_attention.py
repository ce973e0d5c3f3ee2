"""tell/modules/attention/self_attention.py, downsampled_multi_head.py and downsampled_single_head.py on the MI355X
path, in the reference's parameter layout: the entity self-attention of transformer_pointer.

Only the configuration the pointer models build is run: `project_input=False`, no downsampling, 16 heads.  The
attention module's GatedLinear stacks (in_proj_q / in_proj_k / in_proj_v of SingleHeadAttention) exist so that state
dicts match the reference; project_input=False means they are never applied and never receive a gradient."""
import torch.nn as nn

from .. import ops
from .linear import GehringLinear


def GatedLinear(in_features, out_features, dropout=0., bias=True):
    """Weight-normalised linears with interspersed GLUs (downsampled_single_head.py GatedLinear)."""
    return nn.Sequential(
        GehringLinear(in_features, out_features * 4, dropout, bias),
        nn.GLU(),
        GehringLinear(out_features * 2, out_features * 2, dropout, bias),
        nn.GLU(),
        GehringLinear(out_features, out_features, dropout, bias))


class SingleHeadAttention(nn.Module):
    """Parameter holder of downsampled_single_head.py SingleHeadAttention (not downsampled): the projection stacks
    and `out_proj`."""

    def __init__(self, out_channels, embed_dim, head_dim, head_index, dropout=0., bias=True, project_input=True,
                 gated=False, downsample=False, num_heads=1):
        super().__init__()
        assert not downsample, 'the pointer models build the attention without downsampling'
        self.embed_dim, self.head_dim, self.num_heads = embed_dim, head_dim, num_heads
        self.project_input, self.gated, self.dropout = project_input, gated, dropout
        out_proj_size = head_dim * num_heads
        lin = GatedLinear if gated else (lambda i, o, bias=True: GehringLinear(i, o, bias=bias))
        self.in_proj_q = lin(embed_dim, out_proj_size, bias=bias)
        self.in_proj_k = nn.Sequential(lin(embed_dim, out_proj_size, bias=bias))
        self.in_proj_v = nn.Sequential(lin(embed_dim, out_proj_size, bias=bias))
        self.out_proj = GehringLinear(out_proj_size, out_channels, bias=bias)
        self.scaling = head_dim ** -0.5


class DownsampledMultiHeadAttention(nn.ModuleList):
    """downsampled_multi_head.py without downsampling: one SingleHeadAttention over all heads."""

    def __init__(self, out_channels, embed_dim, num_heads, dropout=0., bias=True, project_input=True, gated=False,
                 downsample=False):
        super().__init__()
        assert not downsample and not project_input, 'the pointer models use project_input=False, no downsampling'
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.head_dim = embed_dim // num_heads
        self.attention_module = SingleHeadAttention(out_channels, embed_dim, self.head_dim, 1, dropout, bias,
                                                    project_input, gated, downsample, num_heads)


class SelfAttention(nn.Module):
    """LayerNorm(X + out_proj(attention)), the attention over strictly earlier positions plus a zero slot
    (self_attention.py:26-70 with mask_future_timesteps and use_scalar_bias).  X: [T, B, C]."""

    def __init__(self, out_channels, embed_dim, num_heads, project_input=False, gated=False, downsample=False,
                 weight_norm=True):
        super().__init__()
        self.attention = DownsampledMultiHeadAttention(out_channels, embed_dim, num_heads, dropout=0, bias=True,
                                                       project_input=project_input, gated=gated, downsample=downsample)
        self.in_proj_q = GehringLinear(out_channels, embed_dim, weight_norm=weight_norm)
        self.in_proj_k = GehringLinear(out_channels, embed_dim, weight_norm=weight_norm)
        self.in_proj_v = GehringLinear(out_channels, embed_dim, weight_norm=weight_norm)
        self.ln = nn.LayerNorm(out_channels)

    def _finish(self, attn, X):
        return ops.layer_norm(self.attention.attention_module.out_proj(attn), X, self.ln.weight, self.ln.bias)

    def forward(self, X):
        H = self.attention.num_heads
        am = self.attention.attention_module
        attn = ops.causal_attention(self.in_proj_q(X), self.in_proj_k(X), self.in_proj_v(X), H, am.scaling)
        return self._finish(attn, X)

    def project_kv(self, x):
        return self.in_proj_k(x), self.in_proj_v(x)

    def step(self, x, k_hist, v_hist):
        """The last row of forward() for x [1, B, C] at position T - 1 over the K/V history [T, B, C] (its last row is
        x's own key / value, which the row does not see)."""
        am = self.attention.attention_module
        attn = ops.causal_attention_step(self.in_proj_q(x), k_hist, v_hist, self.attention.num_heads, am.scaling)
        return self._finish(attn, x)
