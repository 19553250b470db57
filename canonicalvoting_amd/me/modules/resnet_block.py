"""``MinkowskiEngine.modules.resnet_block`` (imported at utils/minkunet.py:30).
BasicBlock: relu(norm2(conv2(relu(norm1(conv1(x))))) + (downsample(x) or x)), expansion 1.
Bottleneck: relu(norm3(conv3(relu(norm2(conv2(relu(norm1(conv1(x)))))))) + (downsample(x) or x)) with a 1x1 conv, the 3x3x3
conv that carries the stride and a 1x1 conv to 4 * planes, expansion 4.  Nets built from Bottleneck run by the module path
(MinkUNetBase.forward routes only BasicBlock nets to the one-call program)."""
import torch.nn as nn

from .. import MinkowskiBatchNorm, MinkowskiConvolution, MinkowskiReLU


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1,
                 dimension=3):
        super().__init__()
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                          dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=1, dilation=dilation,
                                          dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        residual = x
        out = self.norm1.forward_fused(self.conv1(x), relu=True)
        if self.downsample is not None:
            residual = self.downsample(x)
        return self.norm2.forward_fused(self.conv2(out), residual=residual.F, relu=True)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, bn_momentum=0.1,
                 dimension=3):
        super().__init__()
        self.conv1 = MinkowskiConvolution(inplanes, planes, kernel_size=1, dimension=dimension)
        self.norm1 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv2 = MinkowskiConvolution(planes, planes, kernel_size=3, stride=stride, dilation=dilation,
                                          dimension=dimension)
        self.norm2 = MinkowskiBatchNorm(planes, momentum=bn_momentum)
        self.conv3 = MinkowskiConvolution(planes, planes * self.expansion, kernel_size=1, dimension=dimension)
        self.norm3 = MinkowskiBatchNorm(planes * self.expansion, momentum=bn_momentum)
        self.relu = MinkowskiReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        residual = x
        out = self.norm1.forward_fused(self.conv1(x), relu=True)
        out = self.norm2.forward_fused(self.conv2(out), relu=True)
        if self.downsample is not None:
            residual = self.downsample(x)
        return self.norm3.forward_fused(self.conv3(out), residual=residual.F, relu=True)
