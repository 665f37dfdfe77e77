"""The geometry of er_pairwise_sorted (include/easyrec_hip.h K8p) without a GPU: the Python mirrors of its grid and its
workspace size against the built library's, inside the envelope and outside it."""
from easyrec_amd.builders import pairwise_loss as pwl


def test_grid_and_workspace_mirrors(built_lib):
  from easyrec_amd import kernels
  lib = kernels.load_library(built_lib)
  for tile in (0,) + pwl.TILES + (512, 3000):
    for B in (1, 1024, 1025, 8192, 8193, 131072, 131073):
      rows, nbytes = lib.er_pairwise_sorted_grid(B, tile), lib.er_pairwise_sorted_workspace_bytes(B, tile)
      assert (rows, nbytes) == (pwl.sorted_grid(B, tile), pwl.sorted_workspace_bytes(B, tile)), (B, tile)
      inside = (tile in pwl.TILES and 1 <= B <= 131072) or (tile == 0 and pwl.fits_sorted(B))
      assert (rows > 0) == (nbytes > 0) == inside, (B, tile)
      if inside:
        T = tile or pwl.DEFAULT_TILE
        G = -(-B // T)
        assert (rows - 1) * 256 < B <= rows * 256 and nbytes == 24 * G * T + 24 * B + 20 * rows
  assert lib.er_pairwise_sorted_grid(8192, 0) == lib.er_pairwise_sorted_grid(8193, 512) == 0
  assert lib.er_pairwise_sorted_grid(8193, 0) == 33 and lib.er_pairwise_sorted_grid(131072, 1024) == 512


def test_the_envelopes_meet_at_8192():
  assert pwl.fits_sorted(8193) and pwl.fits_sorted(131072) and not pwl.fits_sorted(8192) and not pwl.fits_sorted(131073)
  assert pwl.fits(8192) and not pwl.fits(8193) and pwl.MAX_BATCH_SORTED == 131072
