"""The layers reachable from a backbone `keras_layer { class_name: ... }` block
(reference easy_rec/python/layers/keras/__init__.py; located by utils/load_class.load_keras_layer)."""
from .blocks import MLP, Add, Gate, Highway  # noqa: F401
from .interaction import CIN, FM, Cross, DotInteraction  # noqa: F401
from .multi_task import MMoE  # noqa: F401
from .din import DIN  # noqa: F401
from .fibinet import BiLinear, FiBiNet, SENet  # noqa: F401
from .mask_net import MaskBlock, MaskNet  # noqa: F401
from .ppnet import PPNet  # noqa: F401
from .standard import Activation, Dense, Dropout  # noqa: F401
from .text_cnn import TextCNN  # noqa: F401
