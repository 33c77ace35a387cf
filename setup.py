import os
import shutil

from setuptools import find_packages, setup

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from torch.utils.cpp_extension import BuildExtension, CUDAExtension  # noqa: E402


class BuildExt(BuildExtension):
    """ninja records no included file for a .hip source, so an edit to
    a header alone would leave every object as it is.  When a file in
    `depends` is newer than the built extension, the objects go and
    every source is compiled again."""

    def build_extension(self, ext):
        built = self.get_ext_fullpath(ext.name)
        if os.path.exists(built) and any(
                os.path.getmtime(d) > os.path.getmtime(built)
                for d in ext.depends):
            shutil.rmtree(self.build_temp, ignore_errors=True)
        super().build_extension(ext)


ext_modules = [
    CUDAExtension(
        name="hydragnn_amd.ops._hip_ops",
        sources=["hydragnn_amd/ops/csrc/hip_ops.hip",
                 "hydragnn_amd/ops/csrc/etp.hip",
                 "hydragnn_amd/ops/csrc/etp_static.hip",
                 "hydragnn_amd/ops/csrc/mfma_linear.hip",
                 "hydragnn_amd/ops/csrc/varlen_attn.hip",
                 "hydragnn_amd/ops/csrc/gemv.hip",
                 "hydragnn_amd/ops/csrc/radius.hip",
                 "hydragnn_amd/ops/csrc/fused_adamw.hip",
                 "hydragnn_amd/ops/csrc/irreps_linear.hip",
                 "hydragnn_amd/ops/csrc/symcon.hip",
                 "hydragnn_amd/ops/csrc/segment_linear.hip",
                 "hydragnn_amd/ops/csrc/pna_aggr.hip",
                 "hydragnn_amd/ops/csrc/gather_mul.hip",
                 "hydragnn_amd/ops/csrc/painn_message.hip",
                 "hydragnn_amd/ops/csrc/edge_affine.hip",
                 "hydragnn_amd/ops/csrc/edge_affine_mfma.hip",
                 "hydragnn_amd/ops/csrc/act_linear.hip",
                 "hydragnn_amd/ops/csrc/wgrad.hip"],
        # included files: an edit to one rebuilds the extension (BuildExt)
        depends=["hydragnn_amd/ops/csrc/check_launch.h",
                 "hydragnn_amd/ops/csrc/segment_common.h",
                 "hydragnn_amd/ops/csrc/etp_static_tables.inc"],
        extra_compile_args={
            "cxx": ["-O3"],
            "nvcc": ["-O3", "--offload-arch=gfx950"],
        },
    )
]

setup(
    name="hydragnn_amd",
    version="0.1.0",
    description=(
        "MI355X-native multi-headed GNN training framework "
        "(HydraGNN-capability, CDNA4-first)"
    ),
    packages=find_packages(include=["hydragnn_amd", "hydragnn_amd.*"]),
    ext_modules=ext_modules,
    cmdclass={"build_ext": BuildExt.with_options(no_python_abi_suffix=True)},
)
