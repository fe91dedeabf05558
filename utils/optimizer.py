"""`utils.optimizer` of the reference -> cnns_slfp_quantization_amd.optimizer (fused HIP step)."""
from cnns_slfp_quantization_amd.optimizer import *  # noqa: F401,F403
from cnns_slfp_quantization_amd.optimizer import __all__  # noqa: F401
