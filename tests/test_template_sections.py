"""Conditional sections of the kernel templates (codegen.h `select_sections`): the selector on small texts, and what it has to guarantee for
the generated sources -- no marker left, the scene's lines mapped to their owners whatever variant is built, nothing of a variant in the texts
a hand-written kernel pastes in.  No GPU."""
import numpy as np
import pytest

SCENES = ("basics", "portal_in_portal", "monoportal")


def _variants(pa):
    return (0, pa.FLAG_SLICES, pa.FLAG_PASSES, pa.FLAG_SLICES | pa.FLAG_PASSES, pa.FLAG_REFINE, pa.FLAG_REFINE_SLICES)


def _bases(pa):
    return (0, pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL)


TEXT = """head
//%if slices
s1
  //%if passes
s+p
  //%else
s-p
  //%end
s2
//%else
plain
//%if !refine
plain, no refine
//%end
//%end
tail"""


@pytest.mark.parametrize(
    "names, lines",
    [
        ((), ["head", "plain", "plain, no refine", "tail"]),  # a deselected section, its else, a negated condition that holds
        (("refine",), ["head", "plain", "tail"]),  # ... and one that does not
        (("slices",), ["head", "s1", "s-p", "s2", "tail"]),  # a selected section, the else of a nested one
        (("slices", "passes"), ["head", "s1", "s+p", "s2", "tail"]),  # two levels selected
        (("passes", "refine_slices"), ["head", "plain", "plain, no refine", "tail"]),  # the inner name alone selects nothing of a deselected outer section
    ],
)
def test_selector_keeps_exactly_the_lines_of_the_selected_sections(pa, names, lines):
    got = pa.select_sections(TEXT, names)
    assert got == "\n".join(lines)  # (every directive line gone with its newline; the last line had none and has none)
    assert "//%" not in got
    assert pa.select_sections(TEXT + "\n", names) == "\n".join(lines) + "\n"


def test_selector_leaves_a_text_without_directives_alone(pa):
    for text in ("", "\n", "a\n\n  b \n//%slot//%\nc //%if slices\n", "no newline at the end", pa.device_source("glsl"), pa.device_source("refine_entry")):
        for names in ((), ("slices", "passes", "refine", "refine_slices")):
            assert pa.select_sections(text, names) == text


@pytest.mark.parametrize(
    "text, what",
    [
        ("a\n//%if slices\nb\n", "not closed"),
        ("a\n//%if slices\n//%if passes\nb\n//%end\n", "not closed"),
        ("a\n//%end\n", "without an `if`"),
        ("a\n//%else\nb\n//%end\n", "`else` without an `if`"),
        ("//%if slices\na\n//%else\nb\n//%else\nc\n//%end\n", "second `else`"),
        ("//%if sliced\na\n//%end\n", "unknown section name `sliced`"),
        ("//%if !anaglyph\na\n//%end\n", "unknown section name `anaglyph`"),
        ("//%if slices passes\na\n//%end\n", "unknown section name `slices passes`"),  # (one name per condition)
    ],
)
def test_selector_refuses_a_broken_template(pa, text, what):
    with pytest.raises(pa.PortalError, match=what):
        pa.select_sections(text, ("slices",))


def test_selector_refuses_a_name_it_does_not_know_among_the_selected(pa):
    with pytest.raises(pa.PortalError, match="unknown section name `quick`"):
        pa.select_sections("a\n", ("quick",))


@pytest.fixture(scope="module")
def sources(pa):
    """(scene, base, variant) -> (Scene that generated last with these flags, its source)"""
    out = {}
    for name in SCENES:
        for base in _bases(pa):
            for variant in _variants(pa):
                scene = pa.Scene.from_file(pa.scene_path(name))
                out[name, base, variant] = (scene, scene.generate_source(base | variant))
    return out


def test_no_generated_source_keeps_a_marker(pa, sources):
    assert len(sources) == 36
    for key, (_, text) in sources.items():
        assert "//%" not in text, key
    # ... while the template hands its sections and slots out as they are embedded
    assert "//%if slices\n" in pa.device_source("trace") and "//%if passes\n" in pa.device_source("trace") and "//%library//%" in pa.device_source("trace")


def _owned_lines(scene, text):
    lines = text.split("\n")
    owned = []
    for no in range(1, len(lines) + 1):
        owner = scene.source_line_owner(no)
        if owner is not None:
            owned.append((*owner, lines[no - 1]))
    return owned


def test_line_map_names_the_same_scene_lines_in_every_variant(pa, sources):
    """Every line of a generated source that belongs to a scene element -- (owner kind, owner name, line inside the element, the line's text) -- is
    the same list, in the same order, whatever entry variant is built: the sections are selected before the slots are filled, so the map counts
    the lines that are there (the passes build has more lines in front of the snippets than the plain one, and the map follows)."""
    for name in SCENES:
        for base in _bases(pa):
            plain = _owned_lines(*sources[name, base, 0])
            assert len(plain) > 50 and len({o[:2] for o in plain}) >= 2, (name, len(plain))
            for variant in _variants(pa)[1:]:
                assert _owned_lines(*sources[name, base, variant]) == plain, (name, base, variant)
    line_of = lambda text, key: text[:text.index(key)].count("\n")  # noqa: E731
    plain, passes = sources["basics", 0, 0][1], sources["basics", 0, pa.FLAG_PASSES][1]
    assert line_of(passes, "PTL_FN int is_inside_0(") > line_of(plain, "PTL_FN int is_inside_0(")


def test_plain_entry_has_nothing_of_the_variants_and_still_ends_a_handwritten_kernel(pa):
    from oracle import host_build as hb
    from tests import probe

    entry, library = pa.device_source("entry"), pa.device_source("library")
    for text in (entry, library):
        assert "//%" not in text
        for word in ("ptl_slices", "out_passes", "ptl_render_refine", "ptl_pass", "ptl_home", "ptl_host_render_both"):
            assert word not in text, word
    assert "\nptl_render_kernel(unsigned int* __restrict__ out_rgba8," in entry and 'extern "C" unsigned long long ptl_host_render(' in entry
    assert library.count("namespace glsl {\n") == 1 and library.endswith("}  // namespace glsl\n")
    # the one-function kernel of tests/probe.py, host build: three samples through `sqrt` (function 12 of its list)
    assert probe.functions()[12][0] == "sqrt"
    hk = hb.HostKernel(probe.source(pa), probe.LAYOUT, probe.BLOCK_SIZE)
    samples = np.array([[4.0, 0.0, 0.0], [2.25, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    hk.set_texture("in_tex", probe.as_texture(samples))
    hk.set_uniform("n_u", len(samples))
    out = hk.render(len(samples), len(probe.functions()), rgba8=False)["rgba32f"]
    assert out[12, :, 0].tolist() == [2.0, 1.5, 0.0]
