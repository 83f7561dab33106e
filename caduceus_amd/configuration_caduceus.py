"""CaduceusConfig with the reference's field set and defaults
(/root/reference/caduceus/configuration_caduceus.py:10-55), so configs / checkpoints of the reference load unchanged."""
from typing import Optional, Union

from transformers import PretrainedConfig


class CaduceusConfig(PretrainedConfig):
    model_type = "caduceus"

    def __init__(
            self,
            d_model: int = 2560,
            n_layer: int = 64,
            vocab_size: int = 50277,
            ssm_cfg: Optional[dict] = None,
            rms_norm: bool = True,
            residual_in_fp32: bool = True,
            fused_add_norm: bool = True,
            pad_vocab_size_multiple: int = 8,
            norm_epsilon: float = 1e-5,
            initializer_cfg: Optional[dict] = None,
            bidirectional: bool = True,
            bidirectional_strategy: Union[str, None] = "add",
            bidirectional_weight_tie: bool = True,
            rcps: bool = False,
            complement_map: Optional[dict] = None,
            **kwargs,
    ):
        # opt-in fp16 kernels (caduceus_amd.fp16_kernels), not a field of the reference: stored only when given, so that configs without
        # it serialise exactly as before
        fp16_kernels = kwargs.pop("fp16_kernels", None)
        super().__init__(**kwargs)
        if fp16_kernels is not None:
            self.fp16_kernels = bool(fp16_kernels)
        self.d_model = d_model
        self.n_layer = n_layer
        self.vocab_size = vocab_size
        self.ssm_cfg = ssm_cfg
        self.rms_norm = rms_norm
        self.residual_in_fp32 = residual_in_fp32
        self.fused_add_norm = fused_add_norm
        self.pad_vocab_size_multiple = pad_vocab_size_multiple
        self.norm_epsilon = norm_epsilon
        self.initializer_cfg = initializer_cfg
        self.bidirectional = bidirectional
        self.bidirectional_strategy = bidirectional_strategy
        self.bidirectional_weight_tie = bidirectional_weight_tie
        self.rcps = rcps
        # json round-trips turn the int keys of the complement map into strings: normalise (HF from_pretrained path)
        if complement_map is not None:
            complement_map = {int(k): int(v) for k, v in complement_map.items()}
        self.complement_map = complement_map
