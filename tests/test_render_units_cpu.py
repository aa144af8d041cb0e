"""The renderer's translation units (csrc/compile_unit.sh: RENDER_UNITS) between them emit each render kernel exactly once.  A non-template
__global__ function in an anonymous namespace is emitted by every unit whose text contains it, launched there or not, so a kernel defined
in a file that two units include would quietly double the device code.  CPU-only: the kernel names are read from the AMDGPU metadata
notes of the objects the build left in csrc/, the way tools/kernel_resources.py reads them."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'g-nerf_amd', 'csrc')
LLVM = '/opt/rocm/lib/llvm/bin/'


def kernel_names(obj, tmp):
    """Mangled names of the kernels in the gfx950 code object that a hipcc object bundles."""
    fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, 'dev.co')
    subprocess.run([LLVM + 'llvm-objcopy', f'--dump-section=.hip_fatbin={fat}', obj], check=True, capture_output=True)
    subprocess.run([LLVM + 'clang-offload-bundler', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--input={fat}', f'--output={co}', '--unbundle'],
                   check=True, capture_output=True)
    notes = subprocess.run([LLVM + 'llvm-readelf', '--notes', co], check=True, capture_output=True, text=True).stdout
    return re.findall(r'\.name:\s+(\S+)', notes)


def test_every_render_kernel_is_emitted_by_exactly_one_unit(tmp_path):
    units = re.search(r'^RENDER_UNITS="([^"]*)"', open(os.path.join(CSRC, 'compile_unit.sh')).read(), flags=re.M).group(1).split()
    assert 'render' in units and 'render_pipe' in units and len(units) == len(set(units))
    owner, twice = {}, []
    for unit in units:
        obj = os.path.join(CSRC, unit + '.o')
        assert os.path.exists(obj), f'{obj} is missing: csrc/build.sh leaves every unit\'s object there'
        tmp = tmp_path / unit
        tmp.mkdir()
        names = kernel_names(obj, str(tmp))
        assert names and len(names) == len(set(names)), unit
        for name in names:
            if name in owner: twice.append((name, owner[name], unit))
            owner[name] = unit
    assert not twice, f'kernels emitted by two units: {twice}'
    per_unit = {u: sum(1 for o in owner.values() if o == u) for u in units}
    print(per_unit)
    # generic + clamp; 9 + 9 + 6 forward and 3 backward pipelined + tiles + pack; 2 + sorted scatter + 5 binned + ray gradient; 5 point queries
    assert len(owner) == 45, per_unit
