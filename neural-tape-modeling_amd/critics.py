"""The critics of the reference's adversarial training (code/critics.py:125-331, 337-348) on the device: `SpecCrit`,
`MultiSpecCrit`, `DilatedConvDisc` and `get_critic` with the reference's constructor signatures, attribute names and methods.

A SpecCrit is the reference's ModuleList: index 0 the TimeFreqConverter (model.py, the device spectrogram), then real
weight_norm(nn.Conv1d) modules with nn.LeakyReLU(0.2, True) between them at the reference's indices -- so state_dict(), .to(),
parameters(), zero_grad() and an optimizer see what they see in the reference.  forward() does not call those modules: it
hands their weight_g, weight_v and bias to training.SpecCritFn, one graph node for the whole stack on the kernels of
csrc/critic_kernels.hip (the log10 head is read into the first layer).  The mel product stays torch.matmul; the hinge / mean
losses on the outputs and the optimizers stay torch's.  Built: the stride-1 stacks of configs/AdversarialConfig.py's
MultiSpecCrit entries (critic 1, 2 and 5).

A DilatedConvDisc (critic 3: configurations 3 and 7) is the reference's ModuleList in the same way -- weight_norm(nn.Conv1d(...,
dilation=d)) at the even indices, the activation modules at the odd ones -- on the raw waveform; forward() hands the parameters
to training.ConvStackFn, one graph node on the kernels of csrc/convstack_kernels.hip.  Built: nl_func "LeakyReLU" with a
negative_slope in (0, 1), stacks of at most 16 conv layers.

A MelGCrit (get_critic's 'MelGanCrit', critic 0: configurations 0 and 4; code/critics.py:18-122) is the reference's ModuleDict of
NLayerDiscriminator, each a ModuleDict of nn.Sequential(ReflectionPad1d / weight_norm(nn.Conv1d(..., stride, padding, groups)) /
LeakyReLU(0.2, True)) with the reference's keys.  forward() hands the parameters to training.StridedConvStackFn, one graph node per
discriminator on the kernels of csrc/sconv_kernels.hip, and returns what the reference returns: per discriminator the list of
EVERY layer's output (post-activation but for the last: the reference's LeakyReLU is in place), so feature-matching losses
differentiate through all of them.  The reference's loops as they stand: the downsampled signal is dropped (every discriminator
sees the same waveform; the AvgPool1d attribute is kept and not run), and the layer behind the loop takes nf_prev channels, so
only parameter sets where nf_prev == nf there can run -- the others construct, and forward raises."""
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils import weight_norm

from . import training
from .model import TimeFreqConverter

SUPPORTED = ("MultiSpecCrit / SpecCrit with stride=1 (tf_rep 'spec' or 'mel') and DilatedConvDisc with nl_func='LeakyReLU' "
             "(negative_slope in (0, 1)) on a HIP device; MelGanCrit (MelGCrit) with num_D, ndf, n_layers and downsampling_factor "
             "on a HIP device")
MELGAN_PARS = ("num_D", "ndf", "n_layers", "downsampling_factor")


def WNConv1d(*args, **kwargs):
    return weight_norm(nn.Conv1d(*args, **kwargs))


class SpecCrit(nn.Module):
    """Spectral critic that takes the TF representation of audio as input (code/critics.py:181-259)."""

    def __init__(self, scale, kernel_size, hop_size, layers, chan_in, chan_fac, stride, g_fac, tf_rep, log, test_in_len):
        super().__init__()
        if stride != 1:
            raise RuntimeError(f"SpecCrit: stride={stride} has no kernel; supported: {SUPPORTED}")
        if tf_rep not in ("spec", "mel"):
            raise RuntimeError(f"SpecCrit: tf_rep={tf_rep!r}; supported: {SUPPORTED}")
        self.scale = scale
        self.layers = nn.ModuleList()
        self.log = log
        self.log_eps = 1e-5
        self.tf_rep = tf_rep

        self.layers += [TimeFreqConverter(n_fft=scale, hop_length=hop_size, win_length=scale, sampling_rate=44100, n_mel_channels=160)]
        layer1_chan = (scale // 2) + 1 if tf_rep == "spec" else 160
        self.layers += [WNConv1d(in_channels=layer1_chan, out_channels=chan_in, kernel_size=10), nn.LeakyReLU(0.2, True)]
        for _ in range(layers - 2):
            out_channels = min(chan_in * chan_fac, 1024)
            self.layers += [WNConv1d(in_channels=chan_in, out_channels=out_channels, kernel_size=kernel_size, stride=stride,
                                     groups=out_channels // g_fac),
                            nn.LeakyReLU(0.2, True)]
            chan_in = out_channels
        self.layers += [WNConv1d(in_channels=chan_in, out_channels=chan_in, kernel_size=5), nn.LeakyReLU(0.2, True)]
        self.layers += [WNConv1d(in_channels=chan_in, out_channels=1, kernel_size=3)]

        # the reference runs test_input() here: a CPU draw that moves the generator on (a seeded construction must give the
        # next model the reference's weights) and a forward for the printed size.  The draw is made and dropped, the size
        # follows from the sizes: the constructor touches no device
        torch.randn((10, 1, test_in_len))
        print('Spect Disc = {}, kernel size = {}, layers = {}, output size = {},{},{} '
              .format(scale, kernel_size, layers, 10, 1, self.output_frames(test_in_len)))

    def convs(self):
        """The conv modules of the stack, in order."""
        return [m for m in self.layers[1:] if isinstance(m, nn.Conv1d)]

    def spec(self):
        """((c_in, c_out, k, groups), ...) as training.SpecCritFn takes it."""
        return tuple((c.in_channels, c.out_channels, c.kernel_size[0], c.groups) for c in self.convs())

    def output_frames(self, n_samples):
        """Frames of the output for `n_samples` samples of audio."""
        return self.layers[0].n_frames(n_samples) - sum(c.kernel_size[0] - 1 for c in self.convs())

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"SpecCrit: HIP device only (no CPU fallback); supported: {SUPPORTED}")
        if self.tf_rep == 'spec':
            x = self.layers[0](x).squeeze()
        else:
            _, x = self.layers[0](x, mel=True)
            x = x.squeeze()
        if x.dim() not in (2, 3):
            raise RuntimeError(f"SpecCrit: expected (bins, frames) or (batch, bins, frames) behind the transform, got {tuple(x.shape)}")
        params = [p for c in self.convs() for p in (c.weight_g, c.weight_v, c.bias)]
        floor = self.log_eps if self.log else 0.0
        out = training.SpecCritFn.apply(x if x.dim() == 3 else x.unsqueeze(0), floor, self.spec(), *params)
        return out if x.dim() == 3 else out[0]

    def test_input(self, seq_len):
        """The reference's dummy pass: its CPU draw, run where the parameters are."""
        dummy_input = torch.randn((10, 1, seq_len))
        return self(dummy_input.to(self.layers[1].bias.device))


class MultiSpecCrit(nn.Module):
    """Multi-scale container for the spectral critic (code/critics.py:125-178)."""

    def __init__(self, scales, kernel_sizes, hop_sizes, layers, chan_in, chan_fac, stride, g_fac, test_in_len, tf_rep='spec',
                 log=False):
        super().__init__()
        self.scales = scales
        self.models = nn.ModuleList()
        for i in range(len(scales)):
            self.models.append(SpecCrit(scales[i], kernel_sizes[i], hop_sizes[i], layers, chan_in, chan_fac, stride, g_fac, tf_rep,
                                        log, test_in_len))

    def forward(self, x):
        return [model(x) for model in self.models]

    def train_crit(self, fake_ins, real_ins, optimiser):
        D_fake = self(fake_ins)
        D_real = self(real_ins)
        loss_D = 0
        for scale in D_fake:
            loss_D += F.relu(1 + scale).mean()
        for scale in D_real:
            loss_D += F.relu(1 - scale).mean()
        loss_D.backward()
        optimiser.step()
        return loss_D.item()

    def train_gen(self, gen_out, optimiser):
        D_fake = self(gen_out)
        loss_G = 0
        for scale in D_fake:
            loss_G += -scale.mean()
        loss_G.backward()
        optimiser.step()
        return loss_G.item()


class DilatedConvDisc(nn.Module):
    """Time domain crit based on dilated convolutions (code/critics.py:262-331)."""

    def __init__(self, in_channels=1, out_channels=1, kernel_size=5, layers=12, blocks=2, conv_channels=64, dil_fac=2,
                 nl_func="LeakyReLU", nl_params={"negative_slope": 0.2}, test_in_len=1):
        super().__init__()
        if nl_func != "LeakyReLU":
            raise RuntimeError(f"DilatedConvDisc: nl_func={nl_func!r} has no kernel; supported: {SUPPORTED}")
        self.slope = float(nn.LeakyReLU(**nl_params).negative_slope)
        if not 0.0 < self.slope < 1.0:
            raise RuntimeError(f"DilatedConvDisc: LeakyReLU(negative_slope={self.slope}) has no kernel; supported: {SUPPORTED}")
        self.layers = nn.ModuleList()
        # the reference's loops as they stand: range(blocks - 1) builds one block for blocks=2, and the final layer takes
        # in_channels=conv_channels whatever came before it
        for blocks in range(blocks - 1):
            dilation = 1
            for _ in range(layers - 1):
                self.layers += [WNConv1d(in_channels=in_channels, out_channels=conv_channels, kernel_size=kernel_size, dilation=dilation),
                                getattr(nn, nl_func)(**nl_params)]
                dilation *= dil_fac
                in_channels = conv_channels
        self.layers += [WNConv1d(in_channels=conv_channels, out_channels=out_channels, kernel_size=kernel_size, dilation=1)]

        # the reference runs test_input() here: a CPU draw that moves the generator on and a forward for the printed size (which
        # raises where the input is shorter than a kernel's span: its default test_in_len=1 does).  The draw is made and
        # dropped, the size follows from the sizes: the constructor touches no device
        torch.randn((10, 1, test_in_len))
        if test_in_len < self.receptive_field():
            raise RuntimeError(f"DilatedConvDisc: test_in_len={test_in_len} is shorter than the receptive field of "
                               f"{self.receptive_field()} samples")
        print('Dilated Conv Disc, output size = {},{},{} '.format(10, out_channels, self.output_frames(test_in_len)))

    def convs(self):
        """The conv modules of the stack, in order."""
        return [m for m in self.layers if isinstance(m, nn.Conv1d)]

    def spec(self):
        """((c_in, c_out, k, groups, dilation), ...) as training.ConvStackFn takes it."""
        return tuple((c.in_channels, c.out_channels, c.kernel_size[0], c.groups, c.dilation[0]) for c in self.convs())

    def receptive_field(self):
        """Samples of input under one sample of output."""
        return 1 + sum((k - 1) * d for _, _, k, _, d in self.spec())

    def output_frames(self, n_samples):
        """Samples of the output for `n_samples` samples of audio."""
        return n_samples - self.receptive_field() + 1

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"DilatedConvDisc: HIP device only (no CPU fallback); supported: {SUPPORTED}")
        c_in = self.layers[0].in_channels
        if x.dim() not in (2, 3) or x.shape[-2] != c_in:
            raise RuntimeError(f"DilatedConvDisc: expected ({c_in}, samples) or (batch, {c_in}, samples), got {tuple(x.shape)}")
        params = [p for c in self.convs() for p in (c.weight_g, c.weight_v, c.bias)]
        out = training.ConvStackFn.apply(x if x.dim() == 3 else x.unsqueeze(0), self.slope, self.spec(), *params)
        return out if x.dim() == 3 else out[0]

    def train_crit(self, fake_ins, real_ins, optimiser):
        D_fake = self(fake_ins)
        D_real = self(real_ins)
        loss_D = F.relu(1 + D_fake).mean()
        loss_D += F.relu(1 - D_real).mean()
        loss_D.backward()
        optimiser.step()
        return loss_D.item()

    def train_gen(self, gen_out, optimiser):
        D_fake = self(gen_out)
        loss_G = -D_fake.mean()
        loss_G.backward()
        optimiser.step()
        return loss_G.item()

    def test_input(self, seq_len):
        """The reference's dummy pass: its CPU draw, run where the parameters are."""
        dummy_input = torch.randn((10, 1, seq_len))
        return self(dummy_input.to(self.layers[0].bias.device))


def weights_init(m):
    """code/critics.py:364-371.  Under the hook-style weight_norm a Conv1d's `weight` is a plain attribute recomputed from weight_g
    and weight_v before every forward, so the normal_ changes no parameter -- but it draws, and the generator moves on."""
    classname = m.__class__.__name__
    if classname.find("Conv") != -1:
        m.weight.data.normal_(0.0, 0.02)
    elif classname.find("BatchNorm2d") != -1:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0)


class NLayerDiscriminator(nn.Module):
    """Container for multiscale for MelGan critic (code/critics.py:71-122): one discriminator."""

    def __init__(self, ndf, n_layers, downsampling_factor):
        super().__init__()
        model = nn.ModuleDict()
        model["layer_0"] = nn.Sequential(nn.ReflectionPad1d(7), WNConv1d(1, ndf, kernel_size=15), nn.LeakyReLU(0.2, True))
        nf = ndf
        stride = downsampling_factor
        # the reference's loops as they stand: the layer behind the loop takes nf_prev input channels, not nf
        for n in range(1, n_layers + 1):
            nf_prev = nf
            nf = min(nf * stride, 1024)
            model["layer_%d" % n] = nn.Sequential(
                WNConv1d(nf_prev, nf, kernel_size=stride * 10 + 1, stride=stride, padding=stride * 5, groups=nf_prev // 4),
                nn.LeakyReLU(0.2, True))
        nf = min(nf * 2, 1024)
        model["layer_%d" % (n_layers + 1)] = nn.Sequential(WNConv1d(nf_prev, nf, kernel_size=5, stride=1, padding=2),
                                                           nn.LeakyReLU(0.2, True))
        model["layer_%d" % (n_layers + 2)] = WNConv1d(nf, 1, kernel_size=3, stride=1, padding=1)
        self.model = model
        self.slope = 0.2

    def convs(self):
        """The conv modules of the stack, in order."""
        return [m for m in self.model.modules() if isinstance(m, nn.Conv1d)]

    def spec(self):
        """((c_in, c_out, k, groups, stride, pad, pad_mode), ...) as training.StridedConvStackFn takes it: the ReflectionPad1d in
        front of the first conv is its pad with pad_mode 1."""
        out = []
        for layer in self.model.values():
            mods = list(layer) if isinstance(layer, nn.Sequential) else [layer]
            rp = [m for m in mods if isinstance(m, nn.ReflectionPad1d)]
            for c in (m for m in mods if isinstance(m, nn.Conv1d)):
                pad, mode = (int(rp[0].padding[0]), 1) if rp else (int(c.padding[0]), 0)
                out.append((c.in_channels, c.out_channels, c.kernel_size[0], c.groups, c.stride[0], pad, mode))
        return tuple(out)

    def check_chain(self):
        """The reference raises inside conv1d where a layer's input channels are not the output channels in front of it."""
        c = 1
        for n, (c_in, c_out, *_) in enumerate(self.spec()):
            if c_in != c:
                raise RuntimeError(f"NLayerDiscriminator: layer_{n} expects {c_in} input channels and is handed {c} (the layer "
                                   f"behind the strided ones takes the channel count in front of the last of them, as in the "
                                   f"reference); supported: {SUPPORTED}")
            c = c_out

    def output_frames(self, n_samples):
        """Frames of every layer's output for `n_samples` samples of audio."""
        return training._sconvstack_frames(n_samples, self.spec())[1:]

    def forward(self, x):
        self.check_chain()                          # before the device: the reference raises here on any device
        if not x.is_cuda:
            raise RuntimeError(f"NLayerDiscriminator: HIP device only (no CPU fallback); supported: {SUPPORTED}")
        if x.dim() not in (2, 3) or x.shape[-2] != 1:
            raise RuntimeError(f"NLayerDiscriminator: expected (1, samples) or (batch, 1, samples), got {tuple(x.shape)}")
        if x.shape[-1] < 8:
            raise RuntimeError(f"NLayerDiscriminator: ReflectionPad1d(7) needs at least 8 samples, got {x.shape[-1]}")
        params = [p for c in self.convs() for p in (c.weight_g, c.weight_v, c.bias)]
        outs = training.StridedConvStackFn.apply(x if x.dim() == 3 else x.unsqueeze(0), self.slope, self.spec(), *params)
        return list(outs) if x.dim() == 3 else [o[0] for o in outs]


class MelGCrit(nn.Module):
    """Critic from MelGan (code/critics.py:18-68)."""

    def __init__(self, num_D, ndf, n_layers, downsampling_factor):
        super().__init__()
        self.n_layers = n_layers
        self.num_D = num_D
        self.model = nn.ModuleDict()
        for i in range(num_D):
            self.model[f"disc_{i}"] = NLayerDiscriminator(ndf, n_layers, downsampling_factor)
        # kept for named_modules(); the reference runs it and drops the result, so every discriminator sees x: it is not run
        self.downsample = nn.AvgPool1d(4, stride=2, padding=1, count_include_pad=False)
        self.apply(weights_init)

    def forward(self, x):
        for disc in self.model.values():
            disc.check_chain()
        if not x.is_cuda:
            raise RuntimeError(f"MelGCrit: HIP device only (no CPU fallback); supported: {SUPPORTED}")
        return [disc(x) for disc in self.model.values()]

    def train_crit(self, fake_ins, real_ins, optimiser):
        D_fake = self(fake_ins)
        D_real = self(real_ins)
        loss_D = 0
        for scale in D_fake:
            loss_D += F.relu(1 + scale[-1]).mean()
        for scale in D_real:
            loss_D += F.relu(1 - scale[-1]).mean()
        loss_D.backward()
        optimiser.step()
        return loss_D.item()

    def train_gen(self, gen_out, optimiser):
        D_fake = self(gen_out)
        loss_G = 0
        for scale in D_fake:
            loss_G += -scale[-1].mean()
        loss_G.backward()
        optimiser.step()
        return loss_G.item()


def get_critic(critic_name, critic_pars, device, crit_lr, test_in_len):
    """code/critics.py:337-348.  Adam(lr=crit_lr, betas=(0.5, 0.9)) as there, whatever crit_lr is (the configs carry 0)."""
    if critic_name == 'MultiSpecCrit':
        critic_pars['test_in_len'] = test_in_len
        critic = MultiSpecCrit(**critic_pars).to(device=device)
    elif critic_name == 'DilatedConvDisc':
        # no CPU path: an instance on another device could do nothing, so it is refused before anything is built
        if torch.device(device).type != 'cuda':
            raise RuntimeError(f"get_critic: DilatedConvDisc on device {str(device)!r}: HIP device only (no CPU fallback); built: {SUPPORTED}")
        critic_pars['test_in_len'] = test_in_len
        critic = DilatedConvDisc(**critic_pars).to(device=device)
    elif critic_name == 'MelGanCrit':
        missing = [k for k in MELGAN_PARS if k not in critic_pars]
        if missing:
            raise RuntimeError(f"get_critic: {critic_name!r} is not built from critic_pars without {', '.join(missing)}; "
                               f"built: {SUPPORTED}")
        if torch.device(device).type != 'cuda':
            raise RuntimeError(f"get_critic: MelGanCrit on device {str(device)!r}: HIP device only (no CPU fallback); built: {SUPPORTED}")
        critic = MelGCrit(**critic_pars).to(device=device)
    else:
        raise RuntimeError(f"get_critic: {critic_name!r} is not built (MelGanCrit, the strided grouped time-domain critic, is "
                           f"another kernel family); built: {SUPPORTED}")
    optC = torch.optim.Adam(critic.parameters(), lr=crit_lr, betas=(0.5, 0.9))
    return critic, optC
