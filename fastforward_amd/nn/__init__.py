from fastforward_amd.nn.quantizer import Quantizer as Quantizer
from fastforward_amd.nn.quantizer import QuantizerMetadata as QuantizerMetadata
from fastforward_amd.nn.quantizer import QuantizerStub as QuantizerStub
from fastforward_amd.nn.quantizer import Tag as Tag
from fastforward_amd.nn.quantizer import default_tags as default_tags

from fastforward_amd.nn.dynamic_linear_quantizer import DynamicLinearQuantizer as DynamicLinearQuantizer  # isort: skip
from fastforward_amd.nn.linear_quantizer import LinearQuantizer as LinearQuantizer  # isort: skip
from fastforward_amd.nn.lpbq_quantizer import LPBQLinearQuantizer as LPBQLinearQuantizer  # isort: skip
from fastforward_amd.nn.mx_quantizer import MXQuantizer as MXQuantizer  # isort: skip
from fastforward_amd.nn.quantized_module import QuantizedModule as QuantizedModule  # isort: skip
from fastforward_amd.nn.quantized_module import SKIP_QUANTIZATION as SKIP_QUANTIZATION  # isort: skip
from fastforward_amd.nn.quantized_module import named_quantizers as named_quantizers  # isort: skip
from fastforward_amd.nn.quantized_module import quantize_model as quantize_model  # isort: skip
from fastforward_amd.nn.quantized_module import quantized_module_map as quantized_module_map  # isort: skip
from fastforward_amd.nn.quantized_module import surrogate_quantized_modules as surrogate_quantized_modules  # isort: skip
from fastforward_amd.nn import functional as functional  # isort: skip
from fastforward_amd.nn.linear import QuantizedLinear as QuantizedLinear  # isort: skip
from fastforward_amd.nn.container import QuantizedModuleDict as QuantizedModuleDict  # isort: skip
from fastforward_amd.nn.container import QuantizedModuleList as QuantizedModuleList  # isort: skip
from fastforward_amd.nn.container import QuantizedParameterDict as QuantizedParameterDict  # isort: skip
from fastforward_amd.nn.container import QuantizedParameterList as QuantizedParameterList  # isort: skip
from fastforward_amd.nn.container import QuantizedSequential as QuantizedSequential  # isort: skip
from fastforward_amd.nn.normalization import QuantizedLayerNorm as QuantizedLayerNorm  # isort: skip
from fastforward_amd.nn.embedding import QuantizedEmbedding as QuantizedEmbedding  # isort: skip
from fastforward_amd.nn.activations import QuantizedActivation as QuantizedActivation  # isort: skip
from fastforward_amd.nn.activations import QuantizedRelu as QuantizedRelu  # isort: skip
from fastforward_amd.nn.activations import QuantizedSilu as QuantizedSilu  # isort: skip
from fastforward_amd.nn.conv import QuantizedConv1d as QuantizedConv1d  # isort: skip
from fastforward_amd.nn.conv import QuantizedConv2d as QuantizedConv2d  # isort: skip
from fastforward_amd.nn.conv import quantized_conv_modules as quantized_conv_modules  # isort: skip
from fastforward_amd.nn.conv import QuantizedConvTranspose1d as QuantizedConvTranspose1d  # isort: skip
from fastforward_amd.nn.conv import QuantizedConvTranspose2d as QuantizedConvTranspose2d  # isort: skip
from fastforward_amd.nn.conv import quantized_conv_transpose_modules as quantized_conv_transpose_modules  # isort: skip
from fastforward_amd.nn.conv import QuantizedConv3d as QuantizedConv3d  # isort: skip
from fastforward_amd.nn.conv import quantized_conv3d_modules as quantized_conv3d_modules  # isort: skip
from fastforward_amd.nn.kv_cache import QuantizedKVCache as QuantizedKVCache  # isort: skip
from fastforward_amd.nn.kv_cache import PagedQuantizedKVCache as PagedQuantizedKVCache  # isort: skip
from fastforward_amd.nn.kv_cache import DynamicQuantizedKVCache as DynamicQuantizedKVCache  # isort: skip
from fastforward_amd.nn.kv_cache import PagedDynamicQuantizedKVCache as PagedDynamicQuantizedKVCache  # isort: skip
