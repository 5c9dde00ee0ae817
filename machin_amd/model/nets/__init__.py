from .base import (
    NeuralNetworkModule,
    dynamic_module_wrapper,
    static_module_wrapper,
)
from .fused_mlp import FusedMLP
from .gaussian import GaussianPolicyHead
from .iqn import CosineTauEmbedding, ImplicitQuantileHead
from .nature_cnn import ActorCriticCNN, NatureCNN, mlp
from .noisy import (
    NoisyDuelingC51Head,
    NoisyLinear,
    noise_enabled,
    noisy_layers,
    reset_noise,
)
from .resnet import ResNet

__all__ = [
    "NeuralNetworkModule",
    "static_module_wrapper",
    "dynamic_module_wrapper",
    "NatureCNN",
    "ActorCriticCNN",
    "mlp",
    "FusedMLP",
    "ResNet",
    "GaussianPolicyHead",
    "NoisyLinear",
    "NoisyDuelingC51Head",
    "CosineTauEmbedding",
    "ImplicitQuantileHead",
    "reset_noise",
    "noise_enabled",
    "noisy_layers",
]
