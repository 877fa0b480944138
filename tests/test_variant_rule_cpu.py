"""The rule that chooses the env kernels' variant (csrc/orr_variants.h), walked exhaustively without a GPU: all 1024 feature sets at
all five entry points, against a restatement of DESIGN.md section 3's table that is written here and not derived from the header."""
import itertools

import pytest

from tests import variant_probe as vp

PHRASES = {
    "push": "pushes (orr_set_push, orr_bind_push_outputs)",
    "randomizer": "the randomiser (orr_set_randomizer, orr_bind_randomizer_params)",
    "sensor": "sensor noise (orr_set_sensor_noise)",
    "actuator": "torque limits / actuator outputs (orr_set_torque_limits, orr_bind_actuator_outputs)",
    "contacts": "contact outputs (orr_bind_contact_outputs)",
    "terms": "reward terms (orr_bind_reward_terms)",
    "noise": "task noise (orr_set_task_noise)",
    "clips": "a clip set of more than one clip",
}
ORDER = ("push", "randomizer", "sensor", "actuator", "contacts", "terms", "noise", "clips")     # the first that is on decides
VARIANT_OF = {"push": "kPush", "randomizer": "kRandomizer", "sensor": "kSensor", "actuator": "kActuator", "contacts": "kContacts",
              "terms": "kTerms", "noise": "kNoise", "clips": "kClips"}
REPLAYS = ("orr_debug_replay_step", "orr_debug_replay_reset")
ALL_VARIANTS = ("kDefault", "kTwoWave", "kAnchor", "kClips", "kNoise", "kTerms", "kContacts", "kContactsTerms", "kActuator", "kSensor",
                "kRandomizer", "kPush")


def message(entry, feature):
    return "%s: friction anchors (orr_model::friction_anchor) and %s cannot be combined" % (entry, PHRASES[feature])


def expected(on, entry):
    """(variant, message or None) for the set `on` of feature names at `entry`, from the table of DESIGN.md section 3"""
    if entry == "orr_debug_physics":                     # sees contacts and anchors, nothing else; never two waves
        if "contacts" in on:
            return ("kRefused", message(entry, "contacts")) if "anchors" in on else ("kContacts", None)
        return ("kAnchor" if "anchors" in on else "kDefault"), None
    for feature in ORDER:
        if feature not in on or (feature == "contacts" and entry in REPLAYS):      # the replays do not consider contacts at all
            continue
        if "anchors" in on:                              # whether or not the entry point has the variant
            return "kRefused", message(entry, feature)
        if feature == "push" and entry != "orr_step":    # no push variant here: the list goes on
            continue
        if feature == "contacts" and entry == "orr_step" and "terms" in on:
            return "kContactsTerms", None
        return VARIANT_OF[feature], None
    if "anchors" in on:
        return "kAnchor", None
    return ("kTwoWave" if "two_wave" in on else "kDefault"), None


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """{(frozenset of features, entry): (variant, message)} of the probe, for every feature set and entry point"""
    probe = vp.lib(tmp_path_factory)
    assert probe.variants == ALL_VARIANTS
    out = {}
    for bits in itertools.product((False, True), repeat=len(vp.FEATURES)):
        on = frozenset(f for f, b in zip(vp.FEATURES, bits) if b)
        for entry in vp.ENTRIES:
            out[on, entry] = probe.choose(on, entry)
    assert len(out) == 1024 * 5
    return out


def test_every_feature_set_at_every_entry_point(walk):
    wrong = [(sorted(on), entry, got, expected(on, entry)) for (on, entry), got in walk.items() if got != expected(on, entry)]
    assert not wrong, (len(wrong), wrong[:5])


def test_reachable_variants(walk):
    reach = {entry: {v for (_, e), (v, _) in walk.items() if e == entry} for entry in vp.ENTRIES}
    assert reach["orr_step"] == set(ALL_VARIANTS) | {"kRefused"}                   # every variant, at the env step
    for entry in vp.ENTRIES[1:]:
        assert not reach[entry] & {"kPush", "kContactsTerms"}, entry               # and these two nowhere else
    assert reach["orr_debug_physics"] == {"kDefault", "kAnchor", "kContacts", "kRefused"}      # never kTwoWave
    assert "kContacts" not in reach["orr_debug_replay_step"] | reach["orr_debug_replay_reset"]
    # a refusal always names its entry point and one feature; everything else has no message
    for (on, entry), (v, msg) in walk.items():
        assert (msg is not None) == (v == "kRefused")
        if msg:
            assert "anchors" in on and msg.startswith(entry + ": friction anchors (orr_model::friction_anchor) and ") and msg.endswith(" cannot be combined")
