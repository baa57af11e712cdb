"""What the tests of the public headers (capi.HEADERS) share: the functions a header declares, its pedantic C99 / C++11 compile, the C
program that links every declared function and runs the test's own lines, the export tables of the other headers, and what
csrc/Makefile would do, asked of `make` itself (nothing here compiles a kernel or needs a GPU)."""
import functools
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
capi = importlib.import_module("slam-eds_amd.capi")


def declared(header, pattern=r"\b(eds_[A-Za-z0-9_]+)\s*\("):
    """the sorted names that `pattern` finds before a '(' in include/<header>, comments stripped"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(capi.INCLUDE, header)).read(), flags=re.S)
    return sorted(set(re.findall(pattern, text)))


def _includes(headers):
    return [f'#include "{h}"' for h in ([headers] if isinstance(headers, str) else headers)]


def compiles_clean(headers, expr, tmp_path):
    """a main that returns `expr` after the header (or headers) compiles as C99 and as C++11 with warnings as errors"""
    for std, cc, ext in (("-std=c99", "gcc", "c"), ("-std=c++11", "g++", "cpp")):
        src = tmp_path / ("inc." + ext)
        src.write_text("\n".join(_includes(headers)) + f"\nint main(void) {{ return {expr}; }}\n")
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", capi.INCLUDE, "-c", str(src), "-o", str(tmp_path / "inc.o")])


def link_and_run(headers, names, body_lines, tmp_path):
    """a C program takes the address of every function of `names`, runs `body_lines` (each returns its own code on a mismatch) and
    prints the count; it links against libeds_hip.so, runs to 0, and the library defines every name"""
    capi.build()
    lines = ["#include <stdio.h>"] + _includes(headers) + ["int main(void) {", "    const void* f[] = {"]
    lines += [f"        (const void*)(size_t)&{n}," for n in names]
    lines += ["    };", "    size_t i, n = sizeof(f) / sizeof(f[0]);", "    for (i = 0; i < n; ++i) if (!f[i]) return 2;"]
    lines += list(body_lines) + ['    printf("%d functions\\n", (int)n);', "    return 0;", "}"]
    src, exe, libdir = tmp_path / "link.c", tmp_path / "link", os.path.dirname(capi.LIB_PATH)
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", capi.INCLUDE, str(src), "-o", str(exe),
                           "-L", libdir, "-leds_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert f"{len(names)} functions" in subprocess.check_output([str(exe)], text=True)
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    assert set(names) <= set(re.findall(r"\s[TW]\s+(\S+)", out))


def other_exports(exports):
    """every name of every table of capi.HEADERS but `exports` itself"""
    return {n for h in capi.HEADERS if h.exports is not exports for n in h.exports}


@functools.lru_cache(maxsize=None)
def make_commands(*targets):
    """the command lines `make` would run to build `targets` from nothing"""
    return subprocess.check_output(["make", "-n", "-B", "--no-print-directory", "-C", capi.CSRC, *targets], text=True).splitlines()


@functools.lru_cache(maxsize=None)
def make_variable(name):
    """the words of a variable of csrc/Makefile, expanded"""
    db = subprocess.run(["make", "-pnq", "-C", capi.CSRC], capture_output=True, text=True).stdout
    return re.search(rf"^{name} :?= (.*)$", db, re.M).group(1).split()


def is_build_input(name):
    """a file of csrc/ or include/, by its name: `make` holds it in SRCS (a .hip) or HDRS, and capi.build() looks at its age"""
    path = os.path.join(capi.CSRC if os.path.exists(os.path.join(capi.CSRC, name)) else capi.INCLUDE, name)
    known = {os.path.normpath(os.path.join(capi.CSRC, w)) for w in make_variable("SRCS" if name.endswith(".hip") else "HDRS")}
    return os.path.exists(path) and path in known and path in capi.build_inputs()


def compile_line(obj):
    """the one command that makes csrc/<obj>"""
    (line,) = [c for c in make_commands(obj) if c.endswith(" -o " + obj)]
    return line


def resources_line(src):
    """the one command of `make resources` that reports the kernels of csrc/<src>"""
    (line,) = [c for c in make_commands("resources") if f" -c {src} " in c]
    assert "-Rpass-analysis=kernel-resource-usage" in line
    return line


def contraction_off(line):
    """-ffp-contract=off is on the command line and no -ffp-contract=on follows it"""
    return line.rfind("-ffp-contract=off") > line.rfind("-ffp-contract=on")
