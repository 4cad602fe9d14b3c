"""ResNet generator (reference get_generator,
/root/reference/cyclegan/model.py:129-169).

Architecture at defaults (filters=64, 2 down, 9 resblocks, 2 up):
reflect-pad(3) -> conv7x7(64) valid no-bias -> IN -> ReLU
-> [conv3x3 s2 'same' no-bias -> IN -> ReLU] x2 (128, 256)
-> ResBlock(256) x9
-> [convT3x3 s2 'same' no-bias -> IN -> ReLU] x2 (128, 64)
-> reflect-pad(3) -> conv7x7(3) valid bias glorot-init -> tanh

11,383,427 parameters (verified by tests/test_models.py).

``upsample="resize"`` replaces each convT3x3 s2 by nearest-2x upsampling +
conv3x3 'same' (zero pad) — against the transpose conv's checkerboard
artifacts; same parameters, not interchangeable weights.
"""

from __future__ import annotations

import torch.nn as nn

from .layers import (ConvNHWC, ConvTransposeNHWC, InstanceNormNHWC, ResBlock,
                     UpsampleConvNHWC)

# the two upsampling blocks: the reference's stride-2 3x3 transpose conv,
# or nearest-2x upsampling + 3x3 conv (resize-convolution, Odena et al.
# 2016; not in the reference). Same parameter names, shapes and count.
UPSAMPLE_MODES = ("transpose", "resize")


class Generator(nn.Module):
    def __init__(self, in_channels: int = 3, filters: int = 64,
                 num_downsampling_blocks: int = 2, num_residual_blocks: int = 9,
                 num_upsample_blocks: int = 2, upsample: str = "transpose"):
        super().__init__()
        if upsample not in UPSAMPLE_MODES:
            raise ValueError(f"upsample must be one of {UPSAMPLE_MODES}, "
                             f"got {upsample!r}")
        self.upsample = upsample
        f = filters
        self.stem_conv = ConvNHWC(in_channels, f, 7, 1,
                                  padding=(3, 3, 3, 3), pad_mode="reflect")
        self.stem_norm = InstanceNormNHWC(f, act="relu")

        downs = []
        for _ in range(num_downsampling_blocks):
            downs += [ConvNHWC(f, f * 2, 3, 2, padding="same"),
                      InstanceNormNHWC(f * 2, act="relu")]
            f *= 2
        self.downs = nn.ModuleList(downs)

        self.blocks = nn.ModuleList(ResBlock(f) for _ in range(num_residual_blocks))

        ups = []
        for _ in range(num_upsample_blocks):
            up = (UpsampleConvNHWC(f, f // 2) if upsample == "resize"
                  else ConvTransposeNHWC(f, f // 2, 3, 2))
            ups += [up, InstanceNormNHWC(f // 2, act="relu")]
            f //= 2
        self.ups = nn.ModuleList(ups)

        self.head = ConvNHWC(f, in_channels, 7, 1, padding=(3, 3, 3, 3),
                             pad_mode="reflect", bias=True, act="tanh",
                             init="glorot")

    def forward(self, x):
        # fp8 hand-off hints (ops.instance_norm): each norm whose output
        # feeds a resblock conv is told which conv that is — the last down
        # norm -> blocks[0].conv1, block i -> block i+1's conv1; the last
        # block feeds a transpose conv and gets none.
        nb = len(self.blocks)
        h = self.stem_norm(self.stem_conv(x))
        for i, m in enumerate(self.downs):
            if nb and i == len(self.downs) - 1:
                h = m(h, fp8_consumer=self.blocks[0].conv1.fp8_hint())
            else:
                h = m(h)
        for i, b in enumerate(self.blocks):
            nxt = self.blocks[i + 1].conv1.fp8_hint() if i + 1 < nb else None
            h = b(h, fp8_consumer=nxt)
        for m in self.ups:
            h = m(h)
        return self.head(h)
