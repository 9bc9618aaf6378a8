"""What the autograd nodes do with a tensor before a kernel that reads whole rows with 16-byte loads sees it."""


def aligned(t):
    """contiguous AND on a 16-byte boundary: a contiguous view at an odd storage offset -- a slice of a flat buffer -- is copied to a
    fresh allocation instead of being refused by the library (the vector-staging Conv3d launches, both f16x2 backward-weight kernels
    and the pooling kernels take no other pointer).  A tensor that is already both -- every activation the package itself produces
    -- is returned as it is: no copy, no launch."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()
