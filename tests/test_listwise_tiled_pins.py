"""The geometry of er_listwise_tiled (include/easyrec_hip.h K8o) without a GPU: the Python mirrors of its grid and its
workspace size against the built library's, inside the envelope and outside it."""
from easyrec_amd.builders import listwise_loss as lwl


def test_grid_and_workspace_mirrors(built_lib):
  from easyrec_amd import kernels
  lib = kernels.load_library(built_lib)
  for tile in (0,) + lwl.TILES + (512, 3000):
    for B in (1, 1024, 1025, 8192, 8193, 131072, 131073):
      G, nbytes = lib.er_listwise_tiled_grid(B, tile), lib.er_listwise_tiled_workspace_bytes(B, tile)
      assert (G, nbytes) == (lwl.tiled_grid(B, tile), lwl.tiled_workspace_bytes(B, tile)), (B, tile)
      inside = (tile in lwl.TILES and 1 <= B <= 131072) or (tile == 0 and lwl.fits_tiled(B))
      assert (G > 0) == (nbytes > 0) == inside, (B, tile)
      if inside:
        T = tile or lwl.DEFAULT_TILE
        assert (G - 1) * T < B <= G * T and nbytes == 24 * G * T + 64 * G
  assert lib.er_listwise_tiled_grid(8192, 0) == lib.er_listwise_tiled_grid(8193, 512) == lib.er_listwise_tiled_grid(8193, 3000) == 0
  assert lib.er_listwise_tiled_grid(8193, 8192) == 2 and lib.er_listwise_tiled_grid(131072, 1024) == 128
  assert not lwl.tiled_enabled() and lwl.fits_tiled(8193) and not lwl.fits_tiled(8192) and not lwl.fits_tiled(131073)
