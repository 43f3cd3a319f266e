"""Base class for tappable sequential models.

The reference builds a second "transparent" keras model that re-emits chosen
layer outputs (handler_model.py:193-206). In torch we simply return the
intermediate tensors from a single forward pass — the activations never
leave the device, which is the K15 "AT extraction fused into the forward
pass" hot path of the MI355X design (no host round-trip, no second model).
"""

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn


class DropoutTail(NamedTuple):
    """What fused MC-dropout sampling needs from a model whose dropouts all
    sit behind a deterministic attention prefix (``TapModel.dropout_tail``).

    ``embed`` maps the model input to the block input ``x`` [N, T, E];
    ``att`` is the block's ``nn.MultiheadAttention`` (own dropout 0), so
    ``att(x, x, x)[0]`` is the attention output before its dropout;
    ``params`` is an ``ops.McTransformerParams``; ``rates`` holds the four
    dropout rates ``(p_attn, p_ffn, p_pool, p_hidden)``."""

    embed: nn.Module
    att: nn.Module
    params: tuple
    rates: Tuple[float, float, float, float]


class TapModel(nn.Module):
    """A model made of an indexed ``nn.ModuleList`` of layer stages.

    ``forward`` runs the stages in order and returns the final LOGITS
    (softmax is applied by consumers where probabilities are needed — the
    reference's keras models emit softmax directly, argmax semantics are
    identical).
    """

    #: subclasses set: number of classes
    num_classes: int = 0

    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        for layer in self.layers:
            x = layer(x)
        return x

    @torch.no_grad()
    def forward_taps(
        self,
        x: torch.Tensor,
        tap_ids: Optional[Sequence[int]],
        include_output: bool = True,
    ) -> Tuple[List[torch.Tensor], torch.Tensor]:
        """One forward pass, returning ([tapped layer outputs], logits)."""
        taps = []
        wanted = set(tap_ids or [])
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i in wanted:
                taps.append(x)
        if not include_output and wanted:
            pass
        return taps, x

    def has_dropout(self) -> bool:
        """Whether MC-dropout sampling (variation ratio) is applicable."""
        return any(isinstance(m, nn.Dropout) for m in self.modules())

    def dropout_head(self) -> Optional[Tuple[int, float, nn.Linear]]:
        """``(k, p, linear)`` if the model ends in Dropout -> Linear.

        Applies when ``layers[k]`` is an ``nn.Dropout``, ``layers[k+1]`` is
        the final layer and an ``nn.Linear``, and the model holds no other
        ``nn.Dropout`` anywhere. Then all MC-dropout samples of an input
        share the output of ``layers[:k]`` and differ only in the masked
        linear head (``ops.mc_dropout_votes``). Otherwise ``None``.
        """
        k = len(self.layers) - 2
        if k < 0:
            return None
        drop, last = self.layers[k], self.layers[k + 1]
        if not isinstance(drop, nn.Dropout) or not isinstance(last, nn.Linear):
            return None
        if sum(isinstance(m, nn.Dropout) for m in self.modules()) != 1:
            return None
        return k, float(drop.p), last

    def dropout_tail(self) -> Optional[DropoutTail]:
        """A :class:`DropoutTail` if every MC-dropout sample of an input
        shares a deterministic prefix and differs only in a transformer
        block's tail (``ops.mc_transformer_votes``). ``None`` by default."""
        return None
