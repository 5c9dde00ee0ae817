from .classic_control import CartPoleEnv, PendulumEnv, Space, make
from .pixel_catch import PixelCatchEnv
from .pixel_catch_device import DevicePixelCatchVecEnv
from .simple_spread import SimpleSpreadEnv

__all__ = [
    "CartPoleEnv",
    "DevicePixelCatchVecEnv",
    "PendulumEnv",
    "PixelCatchEnv",
    "SimpleSpreadEnv",
    "Space",
    "make",
]
