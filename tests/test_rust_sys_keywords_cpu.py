"""bindings/sys.rs cannot be compiled where the suite runs (no rustc), and the other ABI checks only parse text: a header field or
parameter named like a Rust keyword (`box`, `type`, `ref`, ...) would break the whole `sys` module unnoticed.  Every identifier the
generator emits is checked against the keyword list here, and the generator's own escape is checked on a synthetic header."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# https://doc.rust-lang.org/reference/keywords.html: strict, reserved, and the weak keyword `union`
KEYWORDS = set("""as break const continue crate else enum extern false fn for if impl in let loop match mod move mut pub ref return self Self
static struct super trait true type unsafe use where while async await dyn abstract become box do final macro override priv typeof
unsized virtual yield try union""".split())


def _gen():
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _identifiers(text):
    """(struct field names, function parameter names) of a generated sys.rs"""
    fields = re.findall(r"^    pub (\w+): ", text, flags=re.M)
    params = []
    for plist in re.findall(r"^    pub fn ab_\w+\((.*?)\)(?: -> [^;]+)?;", text, flags=re.M):
        params += re.findall(r"(\w+): ", plist)
    return fields, params


def test_no_generated_field_or_parameter_is_a_rust_keyword():
    text = open(os.path.join(ROOT, "bindings", "sys.rs")).read()
    fields, params = _identifiers(text)
    assert len(fields) > 250 and len(params) > 800, (len(fields), len(params))
    assert "crop_box" in fields
    bad = sorted({n for n in fields + params if n in KEYWORDS})
    assert not bad, f"Rust keywords used as identifiers in bindings/sys.rs: {bad}"
    assert not re.search(r"\br#\w+", text)


def test_the_generator_escapes_keywords_in_fields_and_parameters(tmp_path):
    gen = _gen()
    assert KEYWORDS <= set(gen.RUST_KEYWORDS)
    header = tmp_path / "h.h"
    header.write_text("typedef struct { uint64_t box, type; float ref[3]; int32_t plain; } ab_demo;\n"
                      "AB_API int ab_demo_fn(ab_ctx *ctx, const ab_demo *in, int32_t match, float *move);\n")
    gen.HEADER = str(header)
    text, structs, funcs = gen.generate()
    fields, params = _identifiers(text)
    assert fields == ["box_", "type_", "ref_", "plain"]
    assert params == ["ctx", "in_", "match_", "move_"]
    # the C layout is untouched by the renaming
    size, align, lay = gen.layout(structs, "ab_demo", {})
    assert (size, align, [off for _, off, _ in lay]) == (32, 8, [0, 8, 16, 28])
