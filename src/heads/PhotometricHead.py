"""Plugin-discovery shim for `src.heads.PhotometricHead.Model` (train.py:686-687, eval.py:436-437);
implementation in bihome_amd.heads.PhotometricHead."""
from bihome_amd.heads.PhotometricHead import Model  # noqa: F401
