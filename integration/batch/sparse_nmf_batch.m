function [w, h, objective] = sparse_nmf_batch(vs, p)
% sparse_nmf_batch  [w{k}, h{k}, objective{k}] = sparse_nmf(vs{k}, p) for every matrix of the cell array vs, solved together
% on the GPU in ONE MEX call (integration/snmf_batch_mex.cpp 'solve'; C ABI include/snmf.h: snmf_sparse_nmf_batch_f64 / _fp64,
% and the resident fp64 handle snmf_batch_create_ranks_fp64 / _settings_fp64 for ranks or settings per problem).
%
%   vs   cell array of F x T_k matrices (one F)
%   p    the settings struct of src/sparse_nmf.m, shared by all problems -- or a struct ARRAY with one element per problem
%        (cf / beta, sparsity, max_iter, conv_eps, r, init_w, init_h of its own; cost_check, the masks and random_seed are
%        read from p(1)).  In the shared struct p.r may be a vector (a rank per problem), p.init_w one matrix or a cell
%        array of them, p.init_h a cell array.  A rank or settings per problem need p.snmf_precision = 'fp64'.
%   w, h, objective   cell arrays; objective{k} has the div and cost vectors of the single call (cut at an early stop)
%
% The defaulting and the draws are those of integration/sparse_nmf.m, problem after problem: the reference re-seeds inside
% every sparse_nmf call (rand('seed', p.random_seed)), so every problem starts from the same stream and draws w then h of
% its own shape.  Every problem stops at its own iteration; its results do not depend on the batch around it.
% This file cannot be executed where the project is built: it is unverified beyond the arity of its MEX call.
if nargin < 2, p = struct; end
n = numel(vs);
if n < 1, error('snmf:dim', 'vs must hold at least one matrix'); end
per = numel(p) > 1;
if per && numel(p) ~= n, error('snmf:dim', 'p is a struct array of %d, vs holds %d problems', numel(p), n); end
given = @(q, f) isfield(q, f) && ~isempty(q.(f));

m = size(vs{1}, 1);
T = zeros(n, 1); r = zeros(n, 1); st = zeros(n, 4);
W0 = cell(n, 1); H0 = cell(n, 1);
for k = 1:n
    if size(vs{k}, 1) ~= m, error('snmf:dim', 'problem %d has %d rows, problem 1 has %d', k, size(vs{k}, 1), m); end
    q = p(min(k, numel(p)));
    T(k) = size(vs{k}, 2);
    if ~given(q, 'max_iter'), q.max_iter = 100; end
    if ~given(q, 'random_seed'), q.random_seed = 1; end
    if ~given(q, 'sparsity'), q.sparsity = 0; end
    if ~given(q, 'conv_eps'), q.conv_eps = 0; end
    if ~given(q, 'cf'), q.cf = 'kl'; end
    switch q.cf
        case 'is', q.beta = 0;
        case 'kl', q.beta = 1;
        case 'ed', q.beta = 2;
        otherwise
            if ~given(q, 'beta'), q.beta = 1; end
    end
    if given(q, 'r') && numel(q.r) > 1, q.r = q.r(k); end
    if given(q, 'init_w') && iscell(q.init_w), q.init_w = q.init_w{k}; end
    if given(q, 'init_h') && iscell(q.init_h), q.init_h = q.init_h{k}; end
    % the draws of one sparse_nmf call (src/sparse_nmf.m:112-140): re-seed, then w, then h
    if q.random_seed > 0, rand('seed', q.random_seed); end %#ok<RAND>
    if ~given(q, 'init_w')
        if ~given(q, 'r'), error('Number of components or initialization must be given'); end
        r(k) = q.r;
        W0{k} = rand(m, r(k));
    else
        W0{k} = double(q.init_w);
        r(k) = size(W0{k}, 2);
        if given(q, 'r') && r(k) < q.r
            W0{k} = [W0{k}, rand(m, q.r - r(k))];
            r(k) = q.r;
        end
    end
    if ~given(q, 'init_h')
        H0{k} = rand(r(k), T(k));
    elseif ischar(q.init_h) && strcmp(q.init_h, 'ones')
        H0{k} = ones(r(k), T(k));
    else
        H0{k} = double(q.init_h);
    end
    if per && numel(q.sparsity) > 1, error('snmf:unsupported', 'settings per problem take a scalar sparsity'); end
    st(k, :) = [q.beta, q.sparsity(1), q.conv_eps, q.max_iter];
    if k == 1, q1 = q; end
end

pp = struct('cf', 'beta', 'beta', q1.beta, 'sparsity', double(q1.sparsity), 'max_iter', q1.max_iter, 'conv_eps', q1.conv_eps, ...
            'cost_check', double(p(1).cost_check ~= 0));   % errors like the reference if the field is absent
if all(r == r(1)), pp.r = r(1); else, pp.r = r; end
if given(p(1), 'w_update_ind'), pp.w_update_ind = double(p(1).w_update_ind(:) ~= 0); end
if given(p(1), 'h_update_ind'), pp.h_update_ind = double(p(1).h_update_ind(:) ~= 0); end
if given(p(1), 'snmf_precision'), pp.snmf_precision = char(p(1).snmf_precision); end
if per, settings = st; else, settings = []; end

V = zeros(m, sum(T));
pack = @(c) cell2mat(cellfun(@(a) a(:), c(:), 'UniformOutput', false));
at = 0;
for k = 1:n
    V(:, at + (1:T(k))) = double(vs{k});
    at = at + T(k);
end
[W, H, div, cost, n_iter] = snmf_batch_mex('solve', V, T, pack(W0), pack(H0), pp, settings);

w = cell(n, 1); h = cell(n, 1); objective = cell(n, 1);
aw = 0; ah = 0;
for k = 1:n
    w{k} = W(:, aw + (1:r(k)));
    aw = aw + r(k);
    h{k} = reshape(H(ah + (1:r(k) * T(k))), r(k), T(k));
    ah = ah + r(k) * T(k);
    mi = st(k, 4);
    if ~pp.cost_check
        objective{k} = struct('div', zeros(1, mi), 'cost', zeros(1, mi));
    else
        len = min(n_iter(k), mi);                     % src/sparse_nmf.m:279-280 cut the vectors at an early stop
        objective{k} = struct('div', div(1:len, k)', 'cost', cost(1:len, k)');
    end
end
end
