"""AlphaGo.models.policy_value — see rocalphago_amd/models/policy_value.py."""
from rocalphago_amd.models.policy_value import CNNPolicyValue, ResnetPolicyValue  # noqa: F401
