from .get_magnetic_signed_Laplacian import get_magnetic_signed_Laplacian  # noqa: F401
from .in_out_degree import in_out_degree  # noqa: F401
