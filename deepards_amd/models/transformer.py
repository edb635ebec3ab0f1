"""The cnn_transformer head on MI355X.

Operator surface of reference ``deepards/models/transformer.py`` (MultiHeadAttention :13-56, Block :59-88, Transformer
:91-107) and ``deepards/models/cnn_transformer.py`` (CNNTransformerNetwork :8-44): same constructors, child names,
registration order and ``state_dict`` keys.  The modules are parameter containers: a Block's arithmetic is one fused
kernel forward and two backward (``functional.TransformerBlockFunction``), so ``nn.Linear`` / ``nn.LayerNorm`` /
``nn.Dropout`` children are never called.

Quirks kept: the second residual of a Block adds the block INPUT, not the attended tensor (:88); both dropouts take the
constructor's p (0.2) and are active whenever the module is in training mode -- which the reference's test epoch is too
(train_ards_detector.py:448); ``attention.weights`` holds the last forward's (B, 4, T, T) weights (:52-54).
"""
import torch
import torch.nn as nn

from .. import functional as F_
from .. import hip_ops as H
from .torch_cnn_linear_network import _WindowHead, SEQ_LEN

NUM_HEADS = 4                     # cnn_transformer.py:17: the only head count the reference builds, and the kernels' own


class MultiHeadAttention(nn.Module):
    def __init__(self, input_size, hidden_size, num_heads):
        super(MultiHeadAttention, self).__init__()
        if num_heads != NUM_HEADS:
            raise NotImplementedError('the attention kernels are built for %d heads, got %d' % (NUM_HEADS, num_heads))
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.num_heads = num_heads
        self.head_size = self.hidden_size // num_heads
        self.q_linear = nn.Linear(self.input_size, self.hidden_size)
        self.k_linear = nn.Linear(self.input_size, self.hidden_size)
        self.v_linear = nn.Linear(self.input_size, self.hidden_size)
        self.joint_linear = nn.Linear(self.hidden_size, self.input_size)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, q, k, v):
        raise NotImplementedError('MultiHeadAttention is a parameter container here: the attention runs inside its Block\'s '
                                  'fused kernel (call the Block or the Transformer)')


class Block(nn.Module):
    def __init__(self, input_size, hidden_size, num_heads, activation, dropout):
        super(Block, self).__init__()
        if activation is not nn.ReLU:
            raise NotImplementedError('the feed-forward kernel applies ReLU (the reference\'s default activation)')
        H.tfm_check_shape(1, input_size, hidden_size, 'Block')
        self.dropout = dropout
        self.attention = MultiHeadAttention(input_size, hidden_size, num_heads)
        self.attention_norm = nn.LayerNorm(input_size)
        ff_layers = [nn.Linear(input_size, hidden_size), activation(), nn.Linear(hidden_size, input_size)]
        self.attention_dropout = nn.Dropout(dropout)
        ff_layers.append(nn.Dropout(dropout))
        self.ff = nn.Sequential(*ff_layers)
        self.ff_norm = nn.LayerNorm(input_size)

    def block_params(self):
        """The sixteen tensors in named_parameters() order (the kernels' argument order)."""
        at = self.attention
        mods = (at.q_linear, at.k_linear, at.v_linear, at.joint_linear, self.attention_norm, self.ff[0], self.ff[2],
                self.ff_norm)
        return [t for m in mods for t in (m.weight, m.bias)]

    def forward(self, x, seed=None, salt=0):
        """x (B, T, D) -> (B, T, D).  ``seed``: the Transformer's device-resident dropout seed (``Block.dropout`` > 0 in
        training mode needs it); ``salt``: the first of this block's two mask salts."""
        p = float(self.dropout) if self.training else 0.0
        if p > 0 and seed is None:
            raise RuntimeError('a Block with dropout > 0 in training mode draws its masks from its Transformer\'s seed: call the '
                               'Transformer, or set block.dropout = 0')
        if x.dim() != 3:
            raise ValueError('Block: x must be (B, T, D), got %s' % (tuple(x.shape),))
        H.tfm_check_shape(x.shape[1], x.shape[2], self.attention.hidden_size)
        out, weights = F_.TransformerBlockFunction.apply(x, seed, salt, p, *self.block_params())
        self.attention.weights = weights
        return out


class Transformer(nn.Module):
    def __init__(self, input_size, hidden_size, num_blocks, num_heads, activation=nn.ReLU, dropout=.2):
        super(Transformer, self).__init__()
        self.blocks = nn.Sequential(*[Block(input_size, hidden_size, num_heads, activation, dropout=dropout)
                                      for _ in range(num_blocks)])
        # device-resident dropout seed (as DenseNet's): bumped on the device each forward, so a captured step replays
        # with fresh masks; block i uses the salts 2 i + 1 and 2 i + 2
        self.register_buffer('_drop_seed', torch.zeros(1, dtype=torch.int64), persistent=False)

    def forward(self, x):
        if self.training and any(b.dropout > 0 for b in self.blocks):
            self._drop_seed.add_(0x9E3779B97F4A7C15 >> 1)
        for i, block in enumerate(self.blocks):
            x = block(x, self._drop_seed, 2 * i + 1)
        return x


class CNNTransformerNetwork(_WindowHead):
    """cnn_transformer.py:8-44: breath block -> Transformer over the NB breaths -> Linear(D, 2) per breath -> (B, NB, 2).
    Metadata features are not on the accelerated path (NaN metadata = none, as the reference's default run)."""

    def __init__(self, breath_block, metadata_features, bm_to_linear, hidden_units, num_blocks):
        nn.Module.__init__(self)
        if metadata_features or bm_to_linear:
            raise NotImplementedError('metadata features are outside the accelerated path')
        d = breath_block.n_out_filters
        try:
            H.tfm_check_shape(1, d, hidden_units, 'CNNTransformerNetwork')
        except ValueError as e:
            raise NotImplementedError(str(e))
        self.seq_size = SEQ_LEN
        self.breath_block = breath_block
        self.bm_to_linear = bm_to_linear
        self.transformer = Transformer(d, hidden_units, num_blocks, NUM_HEADS)
        self.linear_final = nn.Linear(d, 2)

    def forward(self, x, metadata):
        b, nb, feat = self._features(x)
        H.tfm_check_shape(nb, feat.shape[1], self.transformer.blocks[0].attention.hidden_size, 'CNNTransformerNetwork')
        y = self.transformer(feat.view(b, nb, feat.shape[1]))
        return self._head(y.reshape(b * nb, -1)).view(b, nb, 2)
