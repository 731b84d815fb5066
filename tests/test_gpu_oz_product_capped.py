"""The capped-lower shape of the int8 products (OzShape::lower_capped: the lower triangle capped
at a number of tile columns, the nested split Cholesky's trapezoid)
through gpe_test_oz_product against tests/oz_product_ref.py's exact integers, with the helpers
and checks of tests/test_gpu_oz_product.py.

The hook takes the form as tri with fewer tile rows in B than in A: B is A's first `cols` rows
(as in chol_schur at q, where one set of planes serves both sides), stored a second time so the
two windows have different leading dimensions.  Everything outside an operand's window is NaN
in its source; C carries a sentinel margin and, inside, the non-zero block the product is
subtracted from (k_oz_crt's accumulate mode, lower128, alpha -1: the production call).

  Rb    cols  K    tiles
  640   256   256  3 tile rows (the last ragged) x 1 column: the smallest trapezoid
  1000  512   128  4 tile rows (the last ragged) x 2 columns: rows 2, 3 past the cap, where the
                   residue tile index changes from the triangle's to cap tiles a row
"""
import numpy as np
import pytest

import oz_product_ref as ozr
import test_gpu_oz_product as top

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Rb,cols,K", [(640, 256, 256), (1000, 512, 128)])
@pytest.mark.parametrize("integer", [0, 1])
def test_form_chol_nest(ctx, Rb, cols, K, integer):
    rng = np.random.default_rng(1000 + Rb + integer)
    l = top._gen(rng, Rb, K, integer)
    ref = ozr.Ref(l, l[:cols], K=K)
    scale = np.ldexp(1.0, -(ref.ea[:, None] + ref.eb[None, :]).astype(np.int32)) * 2.0 ** 106
    a = rng.standard_normal((Rb, cols)) * scale * np.exp2(-rng.integers(0, 60, size=(Rb, cols)).astype(float))
    got = top.run(ctx, top.store(l, 1, ld=Rb + 128), top.store(l[:cols], 1, ld=cols + 64, offset=2), rows=Rb, cols=cols,
                  Cold=a, K=K, tri=1, lower128=1, acc=1, alpha=-1.0)
    top.check("nest Rb=%d cols=%d int=%d" % (Rb, cols, integer), got, ref, rows=Rb, cols=cols, tri=True, lower128=True,
              alpha=-1.0, Cold=a)


def test_capped_needs_tile_row_0(ctx):
    """tri with B shorter than A and ti0 > 0 is no form of the launch layer: GPE_ERR_ARG."""
    a, b = top.store(np.ones((768, 64)), 0), top.store(np.ones((256, 64)), 0)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ctx.test_oz_product(a, b, C=np.zeros(512 * 256), ldc=512, rows=768, cols=256, K=64, tri=1, ti0=1)
