"""mdr_amd — MI355X-native vectorised environment step of marl-demandresponse.

The product path is HIP (libmdr_hip.so, C ABI in include/mdr.h) driven from this Python layer
with PyTorch-ROCm tensors as the device container.  ``import mdr_amd`` does not touch the GPU;
constructing an ``Environment`` loads the library and fails loudly if it (or a GPU) is missing.
"""
from . import config
from .config import EnvironmentProperties

__all__ = ["Environment", "EnvBatch", "EnvironmentProperties", "config", "load_library", "DeviceDQN", "DQNConfig",
           "ReplayStore", "make_qnet", "BatchRolloutStats", "evaluate_batch"]

# names imported on first use (their modules pull in torch): name -> module
_LAZY = {"Environment": "environment", "EnvBatch": "batch", "DeviceDQN": "dqn", "DQNConfig": "dqn", "ReplayStore": "replay",
         "make_qnet": "actor", "BatchRolloutStats": "services", "evaluate_batch": "services"}


def load_library():
    from ._lib import load

    return load()


def __getattr__(name):
    if name in _LAZY:
        import importlib

        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(name)
