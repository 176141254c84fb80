from .toy import HipLinear, toy_model  # noqa: F401
from .resnet import resnet50, ResNet  # noqa: F401
from .vit import (vit_b_16, vit_l_32, vit_tiny,  # noqa: F401
                  VisionTransformer)
from .attention import HipSelfAttention  # noqa: F401
from .layernorm import HipLayerNorm  # noqa: F401
from .mlp import HipMlp  # noqa: F401
from .batchnorm import HipBatchNorm2d  # noqa: F401
from .conv import HipConv2d  # noqa: F401
