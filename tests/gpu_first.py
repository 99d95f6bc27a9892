"""The fixture every GPU test module starts with. A module imports it by name (`from gpu_first import torch_first  # noqa: F401`):
pytest picks an imported fixture up from the importing module's namespace, so it runs once for each module that names it."""
import pytest


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """Bring torch's HIP context up before the library's first call, as the other GPU test modules do."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU: the HIP path has no fallback"
    torch.zeros(1, device="cuda")
