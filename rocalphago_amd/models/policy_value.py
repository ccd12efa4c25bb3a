"""Policy-value network: one convolutional trunk, two heads (beyond the reference, which keeps
a policy and a value network apart; the AlphaGo-Zero-style dual network).

``CNNPolicyValue`` is a registered CNNPolicy subclass, so every policy consumer (players,
``policy_probabilities``, training/search_data.py) takes it as a policy; its second output is
CNNValue's: the expected outcome for the player to move, in [-1, 1]. The functional graph, in
this layer order (trunk parameters first in ``net.flat``):

  InputLayer -> Conv(f1 x f1, relu) -> [Conv(3x3, relu)] x (layers - 1)
     policy: Conv 1x1 (1 filter, linear) -> Flatten -> Bias -> Activation(softmax)      output 0
     value:  Conv 1x1 (1 filter, linear) -> Flatten -> Dense(dense, act) -> Dense(1, tanh)  output 1

On a GPU the whole network runs on the fused HIP plan (models/fused.py DualPlan): one trunk
pass, one head launch for both heads, one backward launch that writes the trunk-top gradient of
both heads once.

``ResnetPolicyValue`` puts the same two heads on ResnetPolicy's residual trunk (its layer list up
to and including the final ReLU; fused.ResnetDualPlan on a GPU). Layers are appended trunk,
policy branch, value branch, so the leading weight arrays are a ResnetPolicy's of the same
arguments.
"""
import numpy as np

from ..features.preprocessing import VALUE_FEATURES
from . import kerasish as K
from .nn_util import Bias, neuralnet
from .policy import CNNPolicy, ResnetPolicy


@neuralnet
class CNNPolicyValue(CNNPolicy):
    """Convolutional policy-value network: state -> (distribution over board points, expected
    outcome for the player to move)."""

    def __init__(self, feature_list=VALUE_FEATURES, **kwargs):
        super(CNNPolicyValue, self).__init__(feature_list, **kwargs)

    def _model_forward(self):
        """The policy output only (numpy [B, S*S]): a drop-in CNNPolicy."""
        model = self.model
        return lambda inpt: model.predict(inpt)[0]

    def forward_device(self, x):
        return self.forward_both_device(x)[0]

    def forward_both_device(self, x):
        """Device-resident batch -> device-resident (probs [B, S*S], values [B])."""
        import torch
        model = self.model
        plan = model._plan_for()
        with torch.no_grad():
            if plan is not None:
                return plan.forward(x)
            p, v = model.net.forward(x.float(), training=False)
            return p, v.reshape(-1)

    def forward_both(self, x):
        """(probs [B, S*S], values [B]) as numpy, from one evaluation of the trunk."""
        p, v = self.model.predict(x)
        return np.asarray(p), np.asarray(v).reshape(-1)

    def batch_eval_value(self, states):
        """CNNValue.batch_eval_state: the value head's output for each state."""
        if len(states) == 0:
            return np.zeros((0,), np.float32)
        return self.forward_both(self.preprocessor.states_to_tensor_u8(states))[1]

    def eval_value(self, state):
        """CNNValue.eval_state: the expected outcome for the player to move."""
        return float(self.forward_both(self.preprocessor.state_to_tensor(state))[1][0])

    @staticmethod
    def create_network(**kwargs):
        """CNNValue's keyword args: input_dim, board (19), filters_per_layer (128),
        filters_per_layer_K, layers (12), filter_width_1 (5), filter_width_K (3), dense (256),
        dense_activation ("relu"), device, seed. No pass logit."""
        params = {"board": 19, "filters_per_layer": 128, "layers": 12, "filter_width_1": 5,
                  "dense": 256, "dense_activation": "relu"}
        params.update(kwargs)
        if params.get("pass_logit"):
            raise ValueError("CNNPolicyValue has no pass logit")
        layers = []

        def add(layer, inbound):
            layer.inbound = list(inbound)
            layers.append(layer)
            return layer.name

        inp = K.Layer("InputLayer", {"name": K._auto_name("input"), "batch_input_shape":
                                     [None, params["input_dim"], params["board"],
                                      params["board"]], "input_dtype": "float32",
                                     "sparse": False})
        layers.append(inp)
        path = add(K.Convolution2D(
            nb_filter=params.get("filters_per_layer_1", params["filters_per_layer"]),
            nb_row=params["filter_width_1"], nb_col=params["filter_width_1"], init='uniform',
            activation='relu', border_mode='same'), [inp.name])
        for i in range(2, params["layers"] + 1):
            fw = params.get("filter_width_%d" % i, 3)
            nf = params.get("filters_per_layer_%d" % i, params["filters_per_layer"])
            path = add(K.Convolution2D(nb_filter=nf, nb_row=fw, nb_col=fw, init='uniform',
                                       activation='relu', border_mode='same'), [path])
        return CNNPolicyValue._two_heads(layers, add, inp, path, params)

    @staticmethod
    def _two_heads(layers, add, inp, path, params):
        """The policy branch (output 0), then the value branch (output 1), on the trunk output
        ``path``; returns the Model."""
        p = add(K.Convolution2D(nb_filter=1, nb_row=1, nb_col=1, init='uniform',
                                border_mode='same'), [path])
        p = add(K.Flatten(), [p])
        p = add(Bias(), [p])
        p = add(K.Activation('softmax'), [p])
        v = add(K.Convolution2D(nb_filter=1, nb_row=1, nb_col=1, init='uniform',
                                activation='linear', border_mode='same'), [path])
        v = add(K.Flatten(), [v])
        v = add(K.Dense(params["dense"], init='uniform',
                        activation=params["dense_activation"]), [v])
        v = add(K.Dense(1, init='uniform', activation='tanh'), [v])
        return K.Model(layers, functional=True, inputs=[inp.name], outputs=[p, v],
                       device=params.get("device"), seed=params.get("seed"))


@neuralnet
class ResnetPolicyValue(CNNPolicyValue):
    """Residual policy-value network: ResnetPolicy's trunk (linear input conv, units of
    n_skip_K x (BatchNorm -> ReLU -> conv) with sum-merge, final ReLU) under CNNPolicyValue's
    two heads."""

    @staticmethod
    def create_network(**kwargs):
        """ResnetPolicy's keyword args: input_dim, board (19), filters_per_layer (128), layers
        (20), filter_width_1 (5), n_skip_K, filter_width_K, bn_axis (-1 column, 1 channel);
        the value head's: dense (256),
        dense_activation ("relu"); device, seed. No pass logit."""
        params = {"board": 19, "filters_per_layer": 128, "layers": 20, "filter_width_1": 5,
                  "dense": 256, "dense_activation": "relu"}
        params.update(kwargs)
        if params.get("pass_logit"):
            raise ValueError("ResnetPolicyValue has no pass logit")
        layers, add, inp, path = ResnetPolicy._trunk(params)
        return CNNPolicyValue._two_heads(layers, add, inp, path, params)
