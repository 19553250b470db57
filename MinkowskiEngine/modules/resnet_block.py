from canonicalvoting_amd.me.modules.resnet_block import BasicBlock, Bottleneck  # noqa: F401
