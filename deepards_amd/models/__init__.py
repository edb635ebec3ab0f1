"""MI355X-native mirror of the reference's ``deepards.models`` operator surface for the cnn_linear
hot path: same constructors, attributes and ``state_dict`` keys."""
from .backbone import Backbone, HEAD_MAP, HEAD_FLAT     # noqa: F401
from .resnet import ResNet, BasicBlock, resnet18, resnet34  # noqa: F401
from .densenet import DenseNet, densenet18, densenet121, densenet169, densenet201       # noqa: F401
from .torch_cnn_linear_network import (CNNLinearNetwork, CNNLinearToMean, CNNLinearComprToRF,      # noqa: F401
                                       CNNSingleBreathLinearNetwork, CNNDoubleLinearNetwork, CNNLSTMNetwork,
                                       BreathBlockLinear)
from .senet import (SENet, SEBasicBlock, SEResNetBottleneck, SEModule, se_resnet18, se_resnet50, se_resnet101,      # noqa: F401
                    se_resnet152)
from .seresnext import se_resnext50_32x4d, se_resnext101_32x4d          # noqa: F401  (the block class stays in its module)
from .vgg import VGG, make_layers, vgg11_bn, vgg13_bn     # noqa: F401
from .transformer import MultiHeadAttention, Block, Transformer, CNNTransformerNetwork           # noqa: F401
from .protopnet1d import (PPNet, construct_PPNet, compute_layer_rf_info, compute_rf_protoL_at_spatial_location,      # noqa: F401
                          compute_rf_prototype, compute_rf_prototypes, compute_proto_layer_rf_info_v2)
from .lstm_only import LSTMOnlyNetwork, LSTMOnlyWithPacking             # noqa: F401
from .siamese import Identity, SiameseCNNLinearNetwork, SiameseCNNLSTMNetwork, SiameseCNNTransformerNetwork         # noqa: F401
from .autoencoder import AutoencoderCNN, AutoencoderNetwork             # noqa: F401  (not a Backbone: no row in the tables below)
from .unet import UNet                                                  # noqa: F401  (the autoencoder route's other base network: no row either)
from .regressor import CNNRegressor                                     # noqa: F401  (breath-metadata pretraining: a head on any Backbone)
from .nested import CNNToNestedRNNNetwork, CNNToNestedLSTMNetwork, CNNToNestedTransformerNetwork        # noqa: F401  (whole-patient heads on densenet18)

# the 1-D BasicBlock / growth-32 entries of the reference's base_networks (train_ards_detector.py:45-69); resnet34 is in
# its models/resnet.py (:178) though not in that dict; se_resnet18 is the SE net its experiment scripts sweep; se_resnet50 /
# 101 / 152 are the bottleneck nets of that dict the reference itself can run (its plain resnet50 / 101 / 152 build their head
# for 8192 features and raise a shape error on the first forward); vgg11 / vgg13 are its vgg11_bn / vgg13_bn (:67-68);
# densenet161 (growth 48), the plain Bottleneck ResNets, the 3x3-stem SE nets (senet18, senet154), the
# VGG nets without BatchNorm and vgg16 / vgg19 are not built
# name -> (factory, class, the group of the driver's build arguments the factory takes -- None: it takes none).  What the
# trainer and the driver decide about a backbone they read from the class's data (models/backbone.py), not from the name.
BACKBONES = {'resnet18': (resnet18, ResNet, 'resnet_kwargs'), 'resnet34': (resnet34, ResNet, 'resnet_kwargs'),
             'densenet18': (densenet18, DenseNet, 'densenet_kwargs'), 'densenet121': (densenet121, DenseNet, 'densenet_kwargs'),
             'densenet169': (densenet169, DenseNet, 'densenet_kwargs'), 'densenet201': (densenet201, DenseNet, 'densenet_kwargs'),
             'se_resnet18': (se_resnet18, SENet, None), 'se_resnet50': (se_resnet50, SENet, None),
             'se_resnet101': (se_resnet101, SENet, None), 'se_resnet152': (se_resnet152, SENet, None),
             'vgg11': (vgg11_bn, VGG, None), 'vgg13': (vgg13_bn, VGG, None)}
base_networks = {name: row[0] for name, row in BACKBONES.items()}
# Backbones built here that the pinned tables above do not list (same rows): the reference's se_resnext50_32x4d /
# se_resnext101_32x4d (train_ards_detector.py:45-69).  backbone_class, build_base_network, the checkpoint loader and the
# driver's --base-network choices consult both tables.
UNLISTED_BACKBONES = {'se_resnext50_32x4d': (se_resnext50_32x4d, SENet, None),
                      'se_resnext101_32x4d': (se_resnext101_32x4d, SENet, None)}


def _row(name):
    return BACKBONES.get(name) or UNLISTED_BACKBONES.get(name)


def backbone_class(name):
    """The class of base network ``name`` (its class data: ``running_stats``, ``bf16_storage``); None for a name not built here."""
    row = _row(name)
    return row[1] if row else None


def build_base_network(name, build_args=None):
    """A fresh base network ``name`` from the driver's build arguments ({'resnet_kwargs': .., 'densenet_kwargs': ..}): the
    factory gets its own group, or nothing."""
    factory, _, group = _row(name) or BACKBONES[name]
    return factory(**((build_args or {}).get(group, {}) if group else {}))
