"""What the numpy models of the pick loop share (csrc/gp_pick.h; DESIGN section 18, "the pick loop"): every inner
product is PARTS sequential sums, which `tree` adds."""

PARTS = 16                 # kPickParts


def tree(parts):
    """The parts added as the balanced tree ((0 + 1) + (2 + 3)) + .. ."""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[2 * q] + parts[2 * q + 1] for q in range(len(parts) // 2)]
    return parts[0]
