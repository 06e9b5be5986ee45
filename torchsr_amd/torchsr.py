"""``torchsr`` command line -- interface of torchsr/torchsr.py:157-270 (same sub-commands, flags
and defaults; ``python -m torchsr_amd.torchsr train ...``).

Differences, all deliberate: the process group backend stays ``nccl`` (= RCCL over xGMI on ROCm)
but falls back to ``gloo`` when no GPU is visible so the launcher itself is testable; the ``test``
sub-command works (the reference's crashes on ``args.seed``); ``--epochs < 8`` no
longer divides by zero; ``--train-dir synthetic:N`` trains on N seeded random crops.
"""
import os
import random
import sys
from argparse import ArgumentParser, ArgumentTypeError, Namespace
from typing import Tuple

import numpy as np
import torch
import torch.distributed as dist

from torchsr_amd.constants import BATCH_SIZE, EPOCHS, MODEL, PRE_EPOCHS, TRAIN_DIR
from torchsr_amd.models import model_names, select_test_model, select_trainer_model

try:  # optional, as in the reference (torchsr.py:26-29)
    import wandb
except ImportError:
    wandb = None


def positive_integer(value: str) -> int:
    """torchsr.py:36-66."""
    try:
        int_value = int(value)
    except (TypeError, ValueError):
        raise ArgumentTypeError(f'invalid int value: \'{value}\'')
    if int_value < 1:
        raise ArgumentTypeError('value must be a positive integer!')
    return int_value


def positive_float(value: str) -> float:
    try:
        float_value = float(value)
    except (TypeError, ValueError):
        raise ArgumentTypeError(f'invalid float value: \'{value}\'')
    if not float_value > 0:  # (also NaN)
        raise ArgumentTypeError('value must be a positive number!')
    return float_value


def probability(value: str) -> float:
    try:
        float_value = float(value)
    except (TypeError, ValueError):
        raise ArgumentTypeError(f'invalid float value: \'{value}\'')
    if not 0.0 <= float_value <= 1.0:  # (also NaN)
        raise ArgumentTypeError('value must be a probability in [0, 1]!')
    return float_value


def ema_decay(value: str) -> float:
    try:
        float_value = float(value)
    except (TypeError, ValueError):
        raise ArgumentTypeError(f'invalid float value: \'{value}\'')
    if not 0.0 <= float_value < 1.0:  # (also NaN)
        raise ArgumentTypeError('value must be a decay in [0, 1)!')
    return float_value


def non_negative_float(value: str) -> float:
    try:
        float_value = float(value)
    except (TypeError, ValueError):
        raise ArgumentTypeError(f'invalid float value: \'{value}\'')
    if not 0.0 <= float_value < float('inf'):  # (also NaN)
        raise ArgumentTypeError('value must be a finite non-negative number!')
    return float_value


def non_negative_integer(value: str) -> int:
    try:
        int_value = int(value)
    except (TypeError, ValueError):
        raise ArgumentTypeError(f'invalid int value: \'{value}\'')
    if int_value < 0:
        raise ArgumentTypeError('value must be a non-negative integer!')
    return int_value


def get_device(args: Namespace) -> torch.device:
    """torchsr.py:69-98."""
    count = torch.cuda.device_count()
    if args.local_world_size > count:
        print('More processes per node requested than GPUs found')
        print('Assuming CPU-only mode... (torchsr_amd has no CPU compute path: train / test need an MI355X and will stop;'
              ' the CPU restatement of the reference lives in oracle/ for tests only)')
        return torch.device('cpu')
    if count < 1 or not torch.cuda.is_available():
        print('No GPUs found')
        print('Running in CPU-only mode... (torchsr_amd has no CPU compute path: train / test need an MI355X and will stop;'
              ' the CPU restatement of the reference lives in oracle/ for tests only)')
        return torch.device('cpu')
    return torch.device('cuda')


def distributed_params(args: Namespace) -> Tuple[Namespace, bool]:
    """torchsr.py:101-154: torchrun env, then Slurm env, else single process (rank -1)."""
    try:
        args.world_size = int(os.environ['WORLD_SIZE'])
        args.rank = int(os.environ['RANK'])
        args.local_rank = int(os.environ['LOCAL_RANK'])
        args.local_world_size = int(os.environ['LOCAL_WORLD_SIZE'])
        distributed = True
    except (KeyError, ValueError):
        try:
            args.world_size = int(os.environ['SLURM_NTASKS'])
            args.rank = int(os.environ['SLURM_PROCID'])
            args.local_rank = int(os.environ['SLURM_LOCALID'])
            args.local_world_size = int(os.environ['SLURM_NTASKS_PER_NODE'])
            os.environ['RANK'] = str(args.rank)
            os.environ['WORLD_SIZE'] = str(args.world_size)
            distributed = True
        except (KeyError, ValueError):
            distributed = False
    if not distributed:
        args.world_size, args.rank, args.local_rank, args.local_world_size = 1, -1, -1, 1
    if getattr(args, 'seed', 0):
        torch.manual_seed(args.seed + args.rank)
    return args, distributed


def parse_args(argv=None) -> Namespace:
    """torchsr.py:157-236."""
    parser = ArgumentParser(description='Super-resolution training and inference on AMD Instinct MI355X')
    commands = parser.add_subparsers(dest='function', metavar='function', required=True)
    train = commands.add_parser('train', help='Train an SRGAN / ESRGAN model against an HD dataset.')
    train.add_argument('--batch-size', type=int, default=BATCH_SIZE)
    train.add_argument('--data-workers', type=positive_integer, default=16)
    train.add_argument('--dataset-multiplier', type=positive_integer, default=1)
    train.add_argument('--disable-amp', action='store_true')
    train.add_argument('--epochs', type=int, default=EPOCHS)
    train.add_argument('--gan-checkpoint', type=str, default=None)
    train.add_argument('--master-addr', type=str, default=None)
    train.add_argument('--master-port', type=str, default=None)
    train.add_argument('--model', type=str, default=MODEL, choices=model_names())
    train.add_argument('--num-conv', type=positive_integer, default=None, metavar='N',
                       help='--model compact only: the number of 64 -> 64 body convs of SRVGGNetCompact (default 32, '
                            'realesr-general-x4v3; realesr-animevideov3 has 16)')
    train.add_argument('--discriminator', type=str, default='vgg', choices=('vgg', 'unet'),
                       help='the critic of the GAN phase.  vgg: the model\'s own VGG-style discriminator with the relativistic '
                            'loss (one logit per crop).  unet: Real-ESRGAN\'s UNetDiscriminatorSN -- a U-Net with spectral '
                            'normalisation and no BatchNorm that returns a logit per pixel -- trained with the plain GAN loss, '
                            'adversarial weight 0.1; --model esrgan and --model compact, one GPU')
    train.add_argument('--perceptual', type=str, default='single', choices=('single', 'realesrgan'),
                       help='the content term of the GAN phase.  single: the reference\'s L1 on VGG19 relu5_4 of the raw images.  '
                            'realesrgan: Real-ESRGAN\'s perceptual loss -- L1 on conv1_2, conv2_2, conv3_4, conv4_4 and conv5_4 '
                            'before their ReLU, weighted 0.1, 0.1, 1, 1, 1, on ImageNet-normalised images -- as one fused node; '
                            '--model esrgan and --model compact, with either --discriminator.  The term\'s weight in the '
                            'generator loss stays 1')
    train.add_argument('--scale', type=int, default=4, choices=(2, 4),
                       help='the factor the generator enlarges by (default 4).  2: RRDBNet behind pixel_unshuffle(2) '
                            '(RealESRGAN_x2plus; --model esrgan) or SRVGGNetCompact with 12 output channels (--model compact); the '
                            'low-resolution side of every training pair is then the crop at 1/2.  --init-generator takes a file '
                            'of this scale only')
    train.add_argument('--pretrain-epochs', type=int, default=PRE_EPOCHS)
    train.add_argument('--psnr-checkpoint', type=str, default=None)
    train.add_argument('--seed', type=int, default=0)
    train.add_argument('--skip-image-save', action='store_true')
    train.add_argument('--train-dir', type=str, default=TRAIN_DIR)
    train.add_argument('--vgg-weights', type=str, default=None,
                       help='path to vgg19-dcbb9e9d.pth (default: $TORCHSR_VGG19_WEIGHTS, then the torch hub cache); '
                            '"random" trains against seeded random VGG19 features (smoke runs only)')
    train.add_argument('--no-graphs', action='store_true', help='run the step eagerly instead of as a hipGraph')
    train.add_argument('--device-data', action='store_true',
                       help='keep the decoded images in HBM and crop / flip / bicubic-downsample on the GPU')
    train.add_argument('--degradation', type=str, default='bicubic', choices=('bicubic', 'blind', 'blind2'),
                       help='how a low-resolution training image is made from its crop.  bicubic: the antialiased bicubic x1/4 '
                            'alone.  blind: anisotropic Gaussian blur, bicubic x1/4, Gaussian noise and JPEG compression with '
                            'parameters drawn per sample (the first-order model of BSRGAN / Real-ESRGAN), all on the GPU.  '
                            'blind2: the second-order model of Real-ESRGAN -- Gaussian, generalised, plateau and sinc kernels, '
                            'resizes by random factors and modes, noise and JPEG, the chain applied twice, then a final sinc '
                            'filter.  blind and blind2 need --device-data: the host DataLoader path has neither.  The per-epoch '
                            'test set stays bicubic')
    train.add_argument('--gt-usm', action='store_true',
                       help='sharpen every training target with Real-ESRGAN\'s unsharp mask (51-tap Gaussian, sigma 8, weight 0.5, '
                            'threshold 10) on the GPU before it is used: the sharpened crop is the target of every loss and the '
                            'input of the selected --degradation.  Needs --device-data.  There is one target per step, so the '
                            'discriminator\'s real sample is the sharpened crop too: Real-ESRNet\'s gt_usm with gan_gt_usm: True, '
                            'where Real-ESRGAN\'s x4plus options set gan_gt_usm: False.  The per-epoch test set is not sharpened')
    train.add_argument('--poisson-noise-prob', type=probability, default=0.0, metavar='FLOAT',
                       help='with --device-data and --degradation blind or blind2: the probability with which a sample of a '
                            'noise stage gets signal-dependent Poisson (shot) noise, the noise of dark photos, in place of the '
                            'stage\'s Gaussian noise.  Real-ESRGAN uses 0.5; the default 0 leaves the degradation as it was')
    train.add_argument('--jpeg-420-prob', type=probability, default=0.0, metavar='FLOAT',
                       help='with --device-data and --degradation blind or blind2: the probability with which a sample of a '
                            'JPEG stage is stored with 4:2:0 chroma subsampling, as nearly every real JPEG is: chroma averaged '
                            '2 x 2, coded in blocks that cover 16 x 16 pixels and interpolated back.  Real-ESRGAN\'s JPEG layer '
                            'always subsamples (1.0); the default 0 leaves the degradation as it was')
    train.add_argument('--pair-pool', type=non_negative_integer, default=0, metavar='N',
                       help='with --device-data and --degradation blind or blind2: keep a pool of N degraded training pairs in HBM '
                            '(Real-ESRGAN\'s training pair pool).  blind2 draws its resize factors, modes and order once per batch; '
                            'with the pool every step stores its fresh pairs in random slots and trains on the pairs it finds '
                            'there, so one step sees several of those draws.  N must be a multiple of --batch-size (Real-ESRGAN: '
                            '180 at batch 12); the first N / batch steps fill the pool and train on their own batches.  The pool is '
                            'per process and is not checkpointed: a resumed run fills it again.  The default 0 is off')
    train.add_argument('--clip-grad-norm', type=positive_float, default=None, metavar='FLOAT',
                       help='clip the global l2 norm of each model\'s gradient to FLOAT before its Adam step '
                            '(torch.nn.utils.clip_grad_norm_, computed on the GPU inside the captured step; default: off)')
    train.add_argument('--skip-nonfinite-steps', action='store_true',
                       help='skip an optimiser step whose gradient holds an inf or a NaN (what the reference\'s GradScaler '
                            'does); the skipped steps are counted and logged per epoch')
    train.add_argument('--init-generator', type=str, default=None, metavar='PATH',
                       help='fine-tune: start the generator from this file -- every format test --weights takes, the published '
                            'RealESRGAN_x4plus / realesr-general-x4v3 files included, in any of their key namings.  The number of '
                            'blocks (--model esrgan) or body convs (--model compact) is read off the file; its scale must be --scale.  '
                            'Optimiser states start at zero.  A phase that finds a checkpoint of its own (--psnr-checkpoint, '
                            '--gan-checkpoint, <model>-{psnr,gan}-latest.pth) resumes from that instead and says so; with '
                            '--pretrain-epochs 0 the GAN phase starts from this file.  --model esrgan and --model compact')
    train.add_argument('--init-discriminator', type=str, default=None, metavar='PATH',
                       help='fine-tune: start the discriminator from this file, loaded strictly: a bare state_dict, '
                            'Real-ESRGAN\'s {"params": ...} (the published *_netD.pth files, with --discriminator unet) or a '
                            'checkpoint of this package (its resume.discriminator entry).  --model esrgan and --model compact')
    train.add_argument('--ema-decay', type=ema_decay, default=None, metavar='FLOAT',
                       help='keep an exponential moving average of the generator\'s weights, ema = FLOAT * ema + (1 - FLOAT) * '
                            'weights after every generator update of both phases, one launch inside the captured step '
                            '(Real-ESRGAN: 0.999).  The averaged weights are what the per-epoch test evaluates, keeps as best / '
                            'latest and shows; every checkpoint gains them as "params_ema" (test --ema runs them).  0 <= FLOAT < 1; '
                            'default: off.  --model esrgan and --model compact')
    train.add_argument('--pixel-weight', type=non_negative_float, default=None, metavar='FLOAT',
                       help='the weight of the L1 term in the GAN phase\'s generator loss (default 0.01, the reference\'s; '
                            'Real-ESRGAN: 1.0).  --model esrgan and --model compact')
    test = commands.add_parser('test', help='Generate a super resolution image from a trained model.')
    test.add_argument('image', type=str)
    test.add_argument('--model', type=str, default=MODEL, choices=model_names())
    test.add_argument('--weights', type=str, default=None, metavar='PATH',
                      help='the checkpoint to load (default: <model>-gan-best.pth in the working directory): a bare state_dict, '
                           'this package\'s {"state": ...} or Real-ESRGAN\'s {"params_ema": ...} / {"params": ...}.  For --model '
                           'compact the number of body convs is read off the file.  --model esrgan takes every published '
                           'RRDBNet file -- RealESRGAN_x4plus, ESRGAN_SRx4_DF2KOST_official, RealESRGAN_x4plus_anime_6B, '
                           'RealESRGAN_x2plus -- in BasicSR / Real-ESRGAN or xinntao/ESRGAN key names as well as this '
                           'package\'s own: the number of blocks and the scale (x4, or x2) are read off the file')
    test.add_argument('--ema', action='store_true',
                      help='run the averaged weights ("params_ema") of a checkpoint written by train --ema-decay instead of its '
                           'live "state"; a file without them is refused')
    test.add_argument('--precision', type=str, default='fp32', choices=('fp32', 'bf16', 'fp16'),
                      help='conv arithmetic of the generator forward: exact fp32 (the reference runs no autocast here), '
                           'bf16 products with fp32 accumulation, or fp16 products and fp16-stored activations with fp32 '
                           'accumulation (SRGAN and compact; an fp16 overflow is reported, not written)')
    test.add_argument('--self-ensemble', type=int, nargs='?', const=8, default=0, choices=(4, 8),
                      help='geometric self-ensemble: run the generator on the 8 flips / transposes of the image (4: the '
                           'flips only), map every result back and average them.  Costs N generator forwards instead of '
                           'one; needs no other weights; combines with every --precision and either --model')
    test.add_argument('--outscale', type=positive_float, default=None, metavar='FLOAT',
                      help='total factor from the image to the result (default: the model\'s own, 4, or 2 for an x2 RRDBNet '
                           'file).  The model always runs at its own scale; its result is then resampled once, on the GPU, '
                           'with the antialiased bicubic filter the training data was reduced with (2 with an x4 model: a 4K '
                           'picture from a 1080p one).  Combines with every --precision, --self-ensemble and every --model')
    test.add_argument('--color-fix', type=str, default=None, choices=('wavelet', 'adain'),
                      help='correct the colour of the model\'s result against the image, on the GPU (default: off).  wavelet: keep '
                           'the result\'s detail and take the low frequencies -- five levels of a dilated 3x3 blur -- from the '
                           'enlarged image; adain: map every channel to the image\'s mean and standard deviation.  Runs behind '
                           'the ensemble average and before --outscale; combines with every other option')
    args = parser.parse_args(argv)
    if args.function == 'train':
        if args.num_conv is not None and args.model.lower() != 'compact':
            parser.error(f'--num-conv sets the depth of --model compact; --model {args.model} has none')
        finetune = args.model.lower() in ('esrgan', 'compact')
        if args.scale != 4 and not finetune:
            parser.error(f'--scale {args.scale} trains with --model esrgan or --model compact; --model {args.model} is the '
                         'reference\'s x4 network, whose two sub-pixel stages have no x2 form')
        for flag, value, why in (('--init-generator', args.init_generator, 'keeps no file format of a published model'),
                                 ('--init-discriminator', args.init_discriminator, 'keeps no file format of a published model'),
                                 ('--ema-decay', args.ema_decay, 'has BatchNorm buffers, which have no average defined'),
                                 ('--pixel-weight', args.pixel_weight, 'has no L1 term in its generator loss')):
            if value is not None and not finetune:
                parser.error(f'{flag} trains with --model esrgan or --model compact; --model {args.model} {why}')
        for flag, value in (('--init-generator', args.init_generator), ('--init-discriminator', args.init_discriminator)):
            if value is not None and not os.path.isfile(value):
                parser.error(f'{flag}: no such file: {value}')
        if args.init_generator is not None and args.model.lower() == 'compact':
            # the file's depth: it sets --num-conv when that was not given, and a --num-conv that differs is an error
            from torchsr_amd.compact.trainer import num_conv_conflict
            from torchsr_amd.test import compact_num_conv, load_generator_state
            try:
                init_state = load_generator_state(args.init_generator)
                depth = compact_num_conv(init_state)
            except Exception as exc:  # (an unreadable file, or not a compact state_dict)
                parser.error(f'--init-generator {args.init_generator}: {exc}')
            if args.num_conv is not None and args.num_conv != depth:
                parser.error(num_conv_conflict(args.num_conv, depth, args.init_generator))
            args.num_conv = depth
            from torchsr_amd.esrgan.trainer import scale_conflict
            from torchsr_amd.test import compact_scale
            try:
                file_scale = compact_scale(init_state, args.init_generator)
            except RuntimeError as exc:
                parser.error(f'--init-generator {exc}')
            if file_scale != args.scale:
                parser.error(scale_conflict(f'--init-generator {args.init_generator}', 'SRVGGNetCompact', file_scale, args.scale))
        if args.num_conv is None:
            args.num_conv = 32
    if args.function == 'train' and args.discriminator == 'unet' and args.model.lower() not in ('esrgan', 'compact'):
        parser.error(f'--discriminator unet trains with --model esrgan or --model compact; --model {args.model} keeps its own '
                     'discriminator')
    if args.function == 'train' and args.perceptual == 'realesrgan' and args.model.lower() not in ('esrgan', 'compact'):
        parser.error(f'--perceptual realesrgan trains with --model esrgan or --model compact; --model {args.model} keeps the '
                     'reference\'s single-layer VGG loss')
    if args.function == 'train' and args.poisson_noise_prob > 0 and not (args.device_data and args.degradation in ('blind', 'blind2')):
        parser.error('--poisson-noise-prob replaces the Gaussian noise of a blind degradation: add --device-data and '
                     '--degradation blind or --degradation blind2')
    if args.function == 'train' and args.jpeg_420_prob > 0 and not (args.device_data and args.degradation in ('blind', 'blind2')):
        parser.error('--jpeg-420-prob subsamples the chroma of a blind degradation\'s JPEG: add --device-data and '
                     '--degradation blind or --degradation blind2')
    if args.function == 'train' and args.pair_pool > 0:
        if not (args.device_data and args.degradation in ('blind', 'blind2')):
            parser.error('--pair-pool pools the pairs of a blind degradation: add --device-data and --degradation blind or '
                         '--degradation blind2')
        if args.batch_size < 1 or args.pair_pool % args.batch_size:
            b = max(args.batch_size, 1)
            nearest = sorted({m for m in (args.pair_pool // b * b, -(-args.pair_pool // b) * b) if m > 0})
            parser.error(f'--pair-pool must be a multiple of --batch-size {args.batch_size} (every step takes a whole batch out of '
                         f'the full pool), got {args.pair_pool}; nearest: {" and ".join(map(str, nearest))}')
    if args.function == 'train' and args.degradation in ('blind', 'blind2') and not args.device_data:
        parser.error(f'--degradation {args.degradation} needs --device-data (the host DataLoader path has no blind degradation)')
    if args.function == 'train' and args.gt_usm and not args.device_data:
        parser.error('--gt-usm needs --device-data (the host DataLoader path has no unsharp mask)')
    return args


def main(argv=None) -> None:
    """torchsr.py:239-270."""
    args = parse_args(argv)
    args, distributed = distributed_params(args)
    model_class = crop_size = None
    if args.function == 'train':
        model_class, crop_size = select_trainer_model(args)
    # checked before wandb.init so that a refused start leaves no open run; a run that never enters the GAN phase
    # (--epochs 0: pre-training only) never evaluates the perceptual loss
    if args.function == 'train' and args.vgg_weights != 'random' and args.epochs > 0:
        # the reference always trains against the pretrained VGG19 (srgan/loss.py:30); a perceptual loss on random
        # features is not that objective, so it has to be asked for
        from torchsr_amd.srgan.loss import VGG19_FILE, _find_weights
        if _find_weights(args.vgg_weights) is None:
            sys.exit(f'torchsr train: {VGG19_FILE} not found (--vgg-weights PATH, $TORCHSR_VGG19_WEIGHTS or the torch hub '
                     'cache); pass "--vgg-weights random" to train against seeded random VGG19 features instead')
    if wandb and args.rank in [-1, 0]:                      # torchsr.py:242-243
        wandb.init(config=args, name='TorchSR', project='torchsr')
    device = get_device(args)
    if args.function == 'test':
        from torchsr_amd.test import test
        test(args, select_test_model(args), device)
        return
    if args.seed:
        random.seed(args.seed)
        np.random.seed(args.seed)
    if distributed:
        if args.master_addr:
            os.environ['MASTER_ADDR'] = args.master_addr
        if args.master_port:
            os.environ['MASTER_PORT'] = args.master_port
        from torchsr_amd.ddp import configure_comm, describe_group
        backend = 'nccl' if device.type == 'cuda' else 'gloo'
        comm = configure_comm(int(args.world_size), backend)  # RCCL channel bounds + CUs left to them, BEFORE the group exists
        args.comm_reserved_cus = comm['reserved_cus_in_comm_window']
        dist.init_process_group(backend=backend)
        if args.rank == 0:
            print(f'process group: {describe_group()}; communication: {comm}')
    args.use_graphs = not args.no_graphs
    from torchsr_amd.dataset import initialize_datasets, initialize_device_datasets
    if args.device_data:
        train_loader, test_loader, train_len, test_len = initialize_device_datasets(
            args.train_dir, device, batch_size=args.batch_size, crop_size=crop_size, upscale_factor=args.scale,
            dataset_multiplier=args.dataset_multiplier, distributed=distributed, seed=args.seed,
            rank=max(int(args.rank), 0) if distributed else 0, world_size=int(args.world_size) if distributed else 1,
            degradation=args.degradation, gt_usm=args.gt_usm, poisson_prob=args.poisson_noise_prob, pair_pool=args.pair_pool,
            jpeg420_prob=args.jpeg_420_prob)
        if args.pair_pool and args.rank in [-1, 0]:
            per_pair = 4 * 3 * (crop_size * crop_size + (crop_size // args.scale) ** 2)
            print(f'training pair pool: {args.pair_pool} pairs per process, {args.pair_pool * per_pair / 1e6:.1f} MB of HBM; the first '
                  f'{args.pair_pool // args.batch_size} steps fill it')
    else:
        train_loader, test_loader, train_len, test_len = initialize_datasets(
            args.train_dir, batch_size=args.batch_size, crop_size=crop_size, upscale_factor=args.scale,
            dataset_multiplier=args.dataset_multiplier, workers=args.data_workers, distributed=distributed,
            seed=args.seed)
    trainer = model_class(device, args, train_loader, test_loader, train_len, test_len, distributed)
    trainer.train()
    if distributed:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
