"""The dealing of claim and walk workgroups with a lead (vh_frame.hip: grouped_role, vh_api_frame.hip: claim_ratio), restated
in a few lines and checked by enumeration: whatever the lead, the claim tiles 0 .. 8 * claimGroups - 1 are each taken once, the
walk ordinals are a bijection of [0, 8 * walkGroups), and a walk ordinal w sits in a workgroup r with w = r (mod 8)."""

M32 = 0xFFFFFFFF


def claim_ratio(claim_groups, span):
    if span == 0 or claim_groups >= span:
        return M32
    return ((claim_groups << 32) + span - 1) // span


def grouped_role(r, claim_blocks, span, ratio, lead):
    """-> (claims, index), with the kernel's 32-bit arithmetic"""
    g = ((r >> 3) - lead) & M32
    q = r & 7
    before = 0 if g >= 1 << 31 else (claim_blocks + 7) >> 3
    if g < span:
        phase = q << 29
        before = ((g * ratio + phase) >> 32) & M32
        after = (((g + 1) * ratio + phase) >> 32) & M32
        if after != before:
            return True, 8 * before + q
    return False, (r - 8 * before) & M32


def check(claim_groups, walk_groups, span, lead, claim_blocks):
    total = claim_groups + walk_groups
    ratio = claim_ratio(claim_groups, span)
    claims, walks = [], []
    for r in range(8 * total):
        is_claim, index = grouped_role(r, claim_blocks, span, ratio, lead)
        if is_claim:
            assert lead <= r >> 3 < lead + span
            claims.append(index)
        else:
            assert index % 8 == r % 8
            walks.append(index)
    assert sorted(claims) == list(range(8 * claim_groups))
    assert sorted(walks) == list(range(8 * walk_groups))


def test_the_lead_keeps_the_dealing_a_bijection_with_the_class_kept():
    cases = 0
    for claim_groups in range(0, 13):
        for walk_groups in range(1, 21):
            total = claim_groups + walk_groups
            # every window the host can choose: strictly more groups than claim groups (claim_span), ending inside the grid
            for span in range(claim_groups + 1, total + 1):
                for lead in range(0, 25):
                    if lead + span > total:
                        break                    # (the host clamps the lead: claim_lead)
                    # the claim tiles of the image: any count that needs claim_groups groups
                    for claim_blocks in ({8 * claim_groups, max(8 * claim_groups - 7, 0)} if claim_groups else {0}):
                        check(claim_groups, walk_groups, span, lead, claim_blocks)
                        cases += 1
    assert cases > 10000


def test_a_lead_beyond_the_grid_is_what_the_clamp_prevents():
    # the restated map itself: a window that starts past the last group deals no claim tile at all, which is why the host clamps
    claims = [r for r in range(8 * 6) if grouped_role(r, 16, 3, claim_ratio(2, 3), 6)[0]]
    assert claims == []
