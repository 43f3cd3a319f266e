"""IMDB text classifier: 1-block transformer.

Mirrors the reference architecture (case_study_imdb.py:48-182): token+position
embedding (dim 32), one transformer block (2 heads, ff 32, post-LN, dropout
0.1), global average pooling, Dense(20, relu), Dense(2). Layer indices match
the keras functional model's ``model.layers`` (InputLayer at 0):
0 input(identity), 1 embedding, 2 transformer block, 3 GAP, 4 dropout,
5 dense20+relu (the SA tap, 20 ATs — reference SA_ACTIVATION_LAYERS=[5]),
6 dropout, 7 dense2. NC taps: [3, 5] (the reference's int-valued entries;
its tuple entries are dead config — see SURVEY.md §2.1).
"""

import torch
import torch.nn as nn

from ..ops.fallback import McTransformerParams
from .base import DropoutTail, TapModel


class TokenAndPositionEmbedding(nn.Module):
    def __init__(self, maxlen: int, vocab_size: int, embed_dim: int):
        super().__init__()
        self.token_emb = nn.Embedding(vocab_size, embed_dim)
        self.pos_emb = nn.Embedding(maxlen, embed_dim)

    def forward(self, x):
        positions = torch.arange(x.shape[-1], device=x.device)
        return self.token_emb(x) + self.pos_emb(positions)


class TransformerBlock(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int, ff_dim: int, rate: float = 0.1):
        super().__init__()
        self.att = nn.MultiheadAttention(embed_dim, num_heads, batch_first=True)
        self.ffn = nn.Sequential(
            nn.Linear(embed_dim, ff_dim), nn.ReLU(), nn.Linear(ff_dim, embed_dim)
        )
        self.layernorm1 = nn.LayerNorm(embed_dim, eps=1e-6)
        self.layernorm2 = nn.LayerNorm(embed_dim, eps=1e-6)
        self.dropout1 = nn.Dropout(rate)
        self.dropout2 = nn.Dropout(rate)

    def forward(self, x):
        attn_out, _ = self.att(x, x, x, need_weights=False)
        x = self.layernorm1(x + self.dropout1(attn_out))
        ffn_out = self.ffn(x)
        return self.layernorm2(x + self.dropout2(ffn_out))


class _GlobalAveragePooling1D(nn.Module):
    def forward(self, x):
        return x.mean(dim=1)


class ImdbTransformer(TapModel):
    """1-block transformer binary sentiment classifier (seq_len 100)."""

    num_classes = 2
    input_shape = (100,)
    sa_layers = [5]
    nc_layers = [3, 5]

    def __init__(self, vocab_size: int = 2000, maxlen: int = 100):
        super().__init__()
        self.layers = nn.ModuleList(
            [
                nn.Identity(),  # keras InputLayer placeholder (index parity)
                TokenAndPositionEmbedding(maxlen, vocab_size, 32),
                TransformerBlock(32, 2, 32),
                _GlobalAveragePooling1D(),
                nn.Dropout(0.1),
                nn.Sequential(nn.Linear(32, 20), nn.ReLU()),
                nn.Dropout(0.1),
                nn.Linear(20, 2),
            ]
        )

    def dropout_tail(self):
        """The embedding stage, the block's attention, the tail's tensors
        and the four dropout rates, when the layer list is exactly
        ``[Identity, embedding, block, pooling, Dropout, Linear + ReLU,
        Dropout, Linear]`` with a dropout-free attention; else ``None``."""
        if len(self.layers) != 8:
            return None
        ident, emb, blk, pool, drop3, dense, drop4, last = self.layers
        if not (
            isinstance(ident, nn.Identity)
            and isinstance(emb, TokenAndPositionEmbedding)
            and isinstance(blk, TransformerBlock)
            and isinstance(pool, _GlobalAveragePooling1D)
            and isinstance(drop3, nn.Dropout)
            and isinstance(dense, nn.Sequential)
            and len(dense) == 2
            and isinstance(dense[0], nn.Linear)
            and isinstance(dense[1], nn.ReLU)
            and isinstance(drop4, nn.Dropout)
            and isinstance(last, nn.Linear)
        ):
            return None
        att, ffn = blk.att, blk.ffn
        if not (
            isinstance(att, nn.MultiheadAttention)
            and att.dropout == 0.0
            and att.batch_first
            and isinstance(ffn, nn.Sequential)
            and len(ffn) == 3
            and isinstance(ffn[0], nn.Linear)
            and isinstance(ffn[1], nn.ReLU)
            and isinstance(ffn[2], nn.Linear)
            and isinstance(blk.layernorm1, nn.LayerNorm)
            and isinstance(blk.layernorm2, nn.LayerNorm)
            and blk.layernorm1.elementwise_affine
            and blk.layernorm2.elementwise_affine
            and blk.layernorm1.eps == blk.layernorm2.eps
            and isinstance(blk.dropout1, nn.Dropout)
            and isinstance(blk.dropout2, nn.Dropout)
        ):
            return None
        linears = (ffn[0], ffn[2], dense[0], last)
        if any(lin.bias is None for lin in linears):
            return None
        if blk.layernorm1.bias is None or blk.layernorm2.bias is None:
            return None
        # the four dropouts named above must be the only ones
        if sum(isinstance(m, nn.Dropout) for m in self.modules()) != 4:
            return None
        params = McTransformerParams(
            blk.layernorm1.weight, blk.layernorm1.bias,
            ffn[0].weight, ffn[0].bias, ffn[2].weight, ffn[2].bias,
            blk.layernorm2.weight, blk.layernorm2.bias,
            float(blk.layernorm1.eps),
            dense[0].weight, dense[0].bias, last.weight, last.bias,
        )
        rates = (
            float(blk.dropout1.p), float(blk.dropout2.p),
            float(drop3.p), float(drop4.p),
        )
        return DropoutTail(emb, att, params, rates)
