"""The recorder's trigger rule restated from the TEXT of include/rmcv_abi.h (the comment above RMCV_TRIG_NO_ARMOURS), in plain Python over
the fields of two loop records: one predicate per bit, a guard per family.  Written from the header's sentences, not from device_loop.h."""
import math

NO_ARMOURS, TRACK_DROPPED, TRACKER_OVF_BIT, FRAME_STATUS, TARGET_LOST, TARGET_SWITCH, NO_SOLUTION, AIM_JUMP, PACKET_ERROR = (1 << b for b in range(9))
AIM_NO_TARGET, AIM_NO_SOLUTION, TRACKER_OVF = 1, 2, 1


def had_target(r):
    return not (r.aim.status & AIM_NO_TARGET)


def solved(r):
    return had_target(r) and not (r.aim.status & AIM_NO_SOLUTION)


def jumped(a, b, bound):
    d = a - b
    if math.isnan(d) or math.isnan(bound):     # "a NaN difference compares false"
        return False
    return abs(d) > bound


ALWAYS = {
    NO_ARMOURS: lambda p, c, cfg: p.n_armours > 0 and c.n_armours == 0,
    TRACK_DROPPED: lambda p, c, cfg: c.n_tracking < p.n_tracking,
    TRACKER_OVF_BIT: lambda p, c, cfg: bool(c.status & TRACKER_OVF) and not (p.status & TRACKER_OVF),
    FRAME_STATUS: lambda p, c, cfg: (c.frame_status & cfg.frame_status_mask & ~p.frame_status) != 0,
}
WITH_AIM_IN_BOTH = {
    TARGET_LOST: lambda p, c, cfg: had_target(p) and bool(c.aim.status & AIM_NO_TARGET),
    TARGET_SWITCH: lambda p, c, cfg: had_target(p) and had_target(c) and c.aim.identity != p.aim.identity,
    NO_SOLUTION: lambda p, c, cfg: bool(c.aim.status & AIM_NO_SOLUTION) and not (p.aim.status & AIM_NO_SOLUTION),
    AIM_JUMP: lambda p, c, cfg: solved(p) and solved(c) and (jumped(c.aim.yaw, p.aim.yaw, cfg.aim_jump_deg) or jumped(c.aim.pitch, p.aim.pitch, cfg.aim_jump_deg)),
}
WITH_ATTITUDE_IN_BOTH = {
    PACKET_ERROR: lambda p, c, cfg: c.packet_errors > p.packet_errors,
}


def trigger(prev, cur, cfg):
    """the bits `cur` raises against `prev`, before the mask"""
    families = [(True, ALWAYS), (bool(prev.has_aim and cur.has_aim), WITH_AIM_IN_BOTH), (bool(prev.has_attitude and cur.has_attitude), WITH_ATTITUDE_IN_BOTH)]
    fired = 0
    for guard, rules in families:
        for bit, rule in rules.items():
            if guard and rule(prev, cur, cfg):
                fired |= bit
    return fired
