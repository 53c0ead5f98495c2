"""FullSystem::trackNewCoarse STEP2-4 (FullSystem.cpp:436-511) in Python, over a mock CoarseTracker that replays event traces.

An independent statement of what csrc/track_tries.h computes: the loop is written as the reference writes it — a tracker object with
lastResiduals / lastFlowIndicators members, called once per try with the running achievedRes — and the tracker's trackNewestCoarse
walks the recorded (lvl, residual, flow) events of that try as CoarseTracker.cpp:1029-1040 would have produced them, returning false at
the first event whose residual exceeds 1.5 * minResForAbort[lvl].  Python floats are IEEE doubles: every comparison here is the
reference's, the casts to float included (numpy.float32)."""
import struct
import warnings

import numpy as np

NAN = float("nan")


def _isfinite_f(x):
    """std::isfinite((float)x)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return bool(np.isfinite(np.float32(x)))


class MockTracker:
    """trackNewestCoarse over a recorded try: dict(events=[(lvl, res, (f0, f1, f2)), ...], end_good, end_pose, end_aff)"""

    def __init__(self):
        self.lastResiduals = [NAN] * 5
        self.lastFlowIndicators = [1000.0] * 3

    def trackNewestCoarse(self, rec, lastToNew, aff_g2l, minResForAbort):
        """-> (good, lastToNew_out, aff_g2l_out, abort_lvl)"""
        self.lastResiduals = [NAN] * 5                           # CoarseTracker.cpp:855
        self.lastFlowIndicators = [1000.0] * 3                   # :856
        for lvl, res, flow in rec["events"]:
            self.lastResiduals[lvl] = res                        # :1029
            self.lastFlowIndicators = list(flow)                 # :1030
            if self.lastResiduals[lvl] > 1.5 * minResForAbort[lvl]:   # :1032
                return False, lastToNew, aff_g2l, lvl
        return bool(rec["end_good"]), rec["end_pose"], rec["end_aff"], -1      # :1044-1068


def track_new_coarse(recs, tries, aff_last_2_l, lastCoarseRMSE, reTrackThreshold, tracker=None):
    """tracker: anything with MockTracker's interface (the GPU tests put the oracle's trackNewestCoarse there; recs[i] is then whatever
    that tracker wants to be handed for try i).
    -> dict(haveOneGood, winner, tryIterations, pose, aff, flowVecs, achievedRes, lastCoarseRMSE, seen=[per try: None (not run) or
    dict(good, abort_lvl, winner, lastResiduals, lastFlowIndicators, pose, aff)])"""
    tracker = tracker or MockTracker()
    flowVecs = [100.0, 100.0, 100.0]                             # :425
    lastF_2_fh = None
    aff_g2l = (0.0, 0.0)
    achievedRes = [NAN] * 5                                      # :436
    haveOneGood = False
    tryIterations = 0
    winner = -1
    seen = [None] * len(tries)
    for i in range(len(tries)):                                  # :441
        aff_g2l_this = aff_last_2_l
        lastF_2_fh_this = tries[i]
        trackingIsGood, lastF_2_fh_this, aff_g2l_this, abort_lvl = tracker.trackNewestCoarse(recs[i], lastF_2_fh_this, aff_g2l_this, achievedRes)
        tryIterations += 1
        took = False
        if trackingIsGood and _isfinite_f(tracker.lastResiduals[0]) and not (tracker.lastResiduals[0] >= achievedRes[0]):   # :475-477
            flowVecs = list(tracker.lastFlowIndicators)
            aff_g2l = aff_g2l_this
            lastF_2_fh = lastF_2_fh_this
            haveOneGood = True
            winner = i
            took = True
        if haveOneGood:                                          # :487-496
            for k in range(5):
                if (not _isfinite_f(achievedRes[k])) or achievedRes[k] > tracker.lastResiduals[k]:
                    achievedRes[k] = tracker.lastResiduals[k]
        seen[i] = dict(good=int(trackingIsGood), abort_lvl=abort_lvl, winner=int(took), lastResiduals=list(tracker.lastResiduals),
                       lastFlowIndicators=list(tracker.lastFlowIndicators), pose=lastF_2_fh_this, aff=aff_g2l_this)
        if haveOneGood and achievedRes[0] < lastCoarseRMSE[0] * reTrackThreshold:   # :499
            break
    if not haveOneGood:                                          # :503-508
        flowVecs = [0.0, 0.0, 0.0]
        aff_g2l = aff_last_2_l
        lastF_2_fh = tries[0]
    return dict(haveOneGood=int(haveOneGood), winner=winner, tryIterations=tryIterations, pose=lastF_2_fh, aff=aff_g2l, flowVecs=flowVecs,
                achievedRes=list(achievedRes), lastCoarseRMSE=list(achievedRes), seen=seen)   # :511


def same_double(a, b):
    """bit for bit (the rules only copy doubles or write the NAN constant, whose bits C and Python share)"""
    return struct.pack("<d", a) == struct.pack("<d", b)
