function B_hats = run_basis_DNMF_batch(xs, ds, Bs, p, mel)
% run_basis_DNMF_batch  B_hats{k} = run_basis_DNMF(xs{k}, ds{k}, Bs{k}, p) for every pair of the cell arrays of waveforms, in ONE
% MEX call on the GPU (integration/snmf_batch_mex.cpp 'dnmf_audio'; C ABI include/snmf.h:
% snmf_run_basis_dnmf_audio_batch_f64 / _fp64 / _ranks_fp64).  With mel = true it is run_basis_DNMF_Mel: the same loop on the
% Mel projections of the three feature sets, Bs{k} then being the Mel bases.
%
%   xs, ds   cell arrays of clean and noise waveforms (any lengths; each pair is cut to its common length)
%   Bs       cell array of [B_x, B_d] bases, F x (R_x(k) + R_d(k)), or one matrix for every pair
%   p        the settings struct; p.R_x / p.R_d may be vectors with one entry per pair (then p.snmf_precision = 'fp64')
%   mel      false (default) or true
%
% What stays here is what must come from MATLAB for RNG parity: the initial activations of solve 1 of every pair, drawn as
% integration/run_basis_DNMF.m draws them -- the reference re-seeds inside every sparse_nmf call, so every pair starts from
% rand('seed', p.random_seed) and draws rand(R_x + R_d, n_frames) of its own shape.  With p.snmf_device_rng = 1 they are
% drawn on the device instead (pair k from the Philox stream keyed by p.random_seed + k - 1).
% This file cannot be executed where the project is built: it is unverified beyond the arity of its MEX calls.
if nargin < 5 || isempty(mel), mel = false; end
if ~isfield(p, 'random_seed'), p.random_seed = 1; end
if isfield(p, 'snmf_precision') && ~isempty(p.snmf_precision), p.snmf_precision = char(p.snmf_precision); end
n = numel(xs);
if numel(ds) ~= n, error('snmf:dim', '%d clean and %d noise waveforms: one of each per pair', n, numel(ds)); end
if ~iscell(Bs), Bs = repmat({Bs}, n, 1); end
R_x = p.R_x(:); R_d = p.R_d(:);
if numel(R_x) == 1, R_x = repmat(R_x, n, 1); end
if numel(R_d) == 1, R_d = repmat(R_d, n, 1); end
r = R_x + R_d;

n_x = zeros(n, 1); n_d = zeros(n, 1); T = zeros(n, 1);
H0 = cell(n, 1);
device_rng = isfield(p, 'snmf_device_rng') && p.snmf_device_rng;
for k = 1:n
    n_x(k) = numel(xs{k}); n_d(k) = numel(ds{k});
    T(k) = snmf_dnmf_mex('nframes', min(n_x(k), n_d(k)), p);
    if ~device_rng
        if p.random_seed > 0, rand('seed', p.random_seed); end %#ok<RAND>
        H0{k} = rand(r(k), T(k));
    end
end
col = @(c) cell2mat(cellfun(@(a) double(a(:)), c(:), 'UniformOutput', false));
if device_rng, H0p = []; else, H0p = col(H0); end
if mel, melmat = mel_matrix(p.fs, p.F_order, p.fftlength, 1, p.fs/2)'; else, melmat = []; end

B_hat = snmf_batch_mex('dnmf_audio', col(xs), n_x, col(ds), n_d, col(Bs), H0p, p, melmat, []);

B_hats = cell(n, 1);
at = 0;
for k = 1:n
    B_hats{k} = B_hat(:, at + (1:r(k)));              % [B_hat_x, B_hat_d], the noise part from column R_x(k) + 1
    at = at + r(k);
end
end
