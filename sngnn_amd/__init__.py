"""sngnn_amd - MI355X-native implementation of SNGNN's similarity-navigated
aggregation path behind the reference's own nn.Module API.

The aggregation runs in hand-written HIP (libsngnn_hip.so, C ABI in
include/sngnn_hip.h); there is no CPU fallback."""
from .acmgcn import ACMGCN, GraphConvolution2
from .conv import AGNNConv, SNConv, SNConv_plus, SNConv_plus_plus
from .gatnet import GAT, GATJK, GATConv
from .gcnii import GCN2Conv, GCNII
from .gcnnet import GCN, GCNJK, GCNConv, MixHop, MixHopLayer
from .ggcn import GGCN, GGCNlayer_SP
from .h2gcnnet import H2GCN, H2GCNConv
from .gpr import APPNP, APPNP_Net, GPR_prop, GPRGNN, MLP
from .linkxnet import LINK, LINK_Concat, LINKX
from .mlpnorm import MLPNORM
from .models import AGNN, SNGNN, SNGNN_Plus, SNGNN_Plus_Plus
from .sgc import SGC, SGCMem, MultiLP
from .synth import Data
from .wrgatnet import WRGAT, WeightedRGATConv

__all__ = ["SNConv", "SNConv_plus", "SNConv_plus_plus", "SNGNN", "SNGNN_Plus",
           "SNGNN_Plus_Plus", "AGNNConv", "AGNN", "GGCNlayer_SP", "GGCN", "MLP", "GPR_prop",
           "GPRGNN", "APPNP", "APPNP_Net", "GATConv", "GAT", "GraphConvolution2", "ACMGCN", "GCN2Conv",
           "GCNII", "GCNConv", "GCN", "GCNJK", "MixHopLayer", "MixHop", "H2GCNConv",
           "H2GCN", "WeightedRGATConv", "WRGAT", "MLPNORM", "LINK", "LINK_Concat", "LINKX", "GATJK", "SGC",
           "SGCMem", "MultiLP", "Data"]
