"""`lpips` as FreeSplat imports it (`from lpips import LPIPS`, src/loss/loss_lpips.py:6 and src/evaluation/metrics.py:6),
backed by freesplat_amd.lpips -- for machines without the third-party package.  Registered in sys.modules under the name
`lpips` only on request (compat.install(lpips=True), `--hip-lpips` of compat.run, or FREESPLAT_LPIPS=hip); it is not
named `lpips` on disk so that a PYTHONPATH entry for freesplat_amd/compat never shadows an installed package."""
from freesplat_amd.lpips import LPIPS  # noqa: F401

__all__ = ["LPIPS"]
